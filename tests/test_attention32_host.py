"""CPU tests of the float32 attention path (the `_t` entry points of include/gca.h, attention.varlen_attention,
gaussiancity_amd.point_attention): the library reports both element types, the typed entry points refuse bad arguments
before they touch the device, the Python layer refuses what varlen_qkvpacked refuses, the emulated float32 contract
(tests/attn_ref32.py) stays within its units, and the backbone binding rebinds, restores and hands every case it does not
fuse to the module's own method."""
import types

import pytest
import torch

import attn_ref32 as R32

GCA_F16, GCA_F32 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from gaussiancity_amd import _native_a as A
    return A.lib()


def test_library_reports_both_dtypes_under_abi_1(lib):
    from gaussiancity_amd import _native_a as A
    from gaussiancity_amd import attention as AT
    assert lib.gca_dtypes() == 3
    assert lib.gca_abi_version() == 1
    for name in ("gca_dtypes", "gca_varlen_forward_t", "gca_varlen_backward_t"):
        assert name in A.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert AT.dtypes() == (torch.float16, torch.float32)


# dummy non-null, 16-byte aligned device addresses, as tests/test_attention_host.py: every call must fail in the checks
def _fwd(lib, dtype=GCA_F32, qkv=16, rs=96, ss=32, hs=16, cu=16, nseg=2, total=64, heads=2, d=16, max_seqlen=32, scale=0.25,
         out=16, lse=16):
    return lib.gca_varlen_forward_t(dtype, qkv, rs, ss, hs, cu, nseg, total, heads, d, max_seqlen, scale, out, lse, None)


def _bwd(lib, dtype=GCA_F32, qkv=16, rs=96, ss=32, hs=16, out=16, dout=16, drs=32, dhs=16, lse=16, cu=16, nseg=2, total=64,
         heads=2, d=16, max_seqlen=32, scale=0.25, dqkv=16, ws=16, ws_bytes=64 * 2 * 4):
    return lib.gca_varlen_backward_t(dtype, qkv, rs, ss, hs, out, dout, drs, dhs, lse, cu, nseg, total, heads, d, max_seqlen,
                                     scale, dqkv, ws, ws_bytes, None)


@pytest.mark.parametrize("dtype", [GCA_F16, GCA_F32])
def test_typed_forward_rejects_bad_arguments_before_touching_the_device(lib, dtype):
    f = lambda **kw: _fwd(lib, dtype, **kw)  # noqa: E731
    for bad in (-1, 2, 7):
        assert _fwd(lib, bad) < 0 and b"dtype" in lib.gca_last_error()
        assert _fwd(lib, bad, total=0) < 0 and b"dtype" in lib.gca_last_error()
    assert f(qkv=None) < 0 and b"null" in lib.gca_last_error()
    assert f(out=None) < 0 and b"null" in lib.gca_last_error()
    assert f(lse=None) < 0
    assert f(cu=None) < 0 and b"cu_seqlens" in lib.gca_last_error()
    assert f(heads=0) < 0 and b"heads" in lib.gca_last_error()
    assert f(heads=-3) < 0
    for d in (0, 8, 24, 48, 128):
        assert f(d=d) < 0 and b"head_dim must be 16, 32 or 64" in lib.gca_last_error()
    assert f(total=-1) < 0 and b"total" in lib.gca_last_error()
    assert f(max_seqlen=-1) < 0 and b"max_seqlen" in lib.gca_last_error()
    assert f(nseg=-1) < 0 and b"nseg" in lib.gca_last_error()
    assert f(rs=0) < 0 and b"strides" in lib.gca_last_error()
    assert f(hs=6) < 0 and b"strides" in lib.gca_last_error()
    assert f(qkv=8) < 0 and b"aligned" in lib.gca_last_error()
    assert f(out=24) < 0 and b"aligned" in lib.gca_last_error()
    assert f(scale=float("nan")) < 0 and b"softmax_scale" in lib.gca_last_error()
    assert f(nseg=2 ** 30, max_seqlen=2 ** 20, total=2 ** 30) < 0 and b"grid" in lib.gca_last_error()
    assert f(total=0, qkv=None, out=None, lse=None, cu=None) == 0      # an empty problem is no error


@pytest.mark.parametrize("dtype", [GCA_F16, GCA_F32])
def test_typed_backward_rejects_bad_arguments_before_touching_the_device(lib, dtype):
    b = lambda **kw: _bwd(lib, dtype, **kw)  # noqa: E731
    for bad in (-1, 2):
        assert _bwd(lib, bad) < 0 and b"dtype" in lib.gca_last_error()
    for name in ("qkv", "out", "dout", "lse", "dqkv"):
        assert b(**{name: None}) < 0 and b"null" in lib.gca_last_error(), name
    assert b(cu=None) < 0 and b"cu_seqlens" in lib.gca_last_error()
    assert b(heads=0) < 0 and b"heads" in lib.gca_last_error()
    assert b(d=20) < 0 and b"head_dim" in lib.gca_last_error()
    assert b(total=-5) < 0 and b"total" in lib.gca_last_error()
    assert b(max_seqlen=-1) < 0 and b"max_seqlen" in lib.gca_last_error()
    assert b(nseg=-1) < 0 and b"nseg" in lib.gca_last_error()
    assert b(drs=6) < 0 and b"strides" in lib.gca_last_error()
    assert b(dhs=0) < 0 and b"strides" in lib.gca_last_error()
    assert b(rs=6) < 0 and b"strides" in lib.gca_last_error()
    for name in ("qkv", "out", "dout", "dqkv"):
        assert b(**{name: 8}) < 0 and b"aligned" in lib.gca_last_error(), name
    assert b(scale=float("inf")) < 0 and b"softmax_scale" in lib.gca_last_error()
    assert b(ws=None) < 0 and b"workspace" in lib.gca_last_error()
    need = lib.gca_backward_workspace_bytes(64, 2)
    assert need == 64 * 2 * 4                                          # D only, whatever the element type
    assert b(ws_bytes=need - 1) < 0 and b"workspace" in lib.gca_last_error()
    assert b(nseg=2 ** 30, max_seqlen=2 ** 20, total=2 ** 30, ws_bytes=2 ** 40) < 0 and b"grid" in lib.gca_last_error()
    assert b(total=0, qkv=None, dqkv=None, ws=None, ws_bytes=0) == 0


def test_float32_stride_rule_is_multiples_of_4(lib):
    assert _fwd(lib, GCA_F32, hs=6) < 0 and b"multiples of 4" in lib.gca_last_error()
    assert _fwd(lib, GCA_F16, hs=12) < 0 and b"multiples of 8" in lib.gca_last_error()
    assert _bwd(lib, GCA_F32, drs=6) < 0 and b"multiples of 4" in lib.gca_last_error()
    # 12 = 3 * 4 is a float32 stride: the call gets past the stride rule and fails on the next check it cannot pass
    assert _fwd(lib, GCA_F32, hs=12, qkv=8) < 0 and b"aligned" in lib.gca_last_error()
    assert _bwd(lib, GCA_F32, dhs=12, dout=8) < 0 and b"aligned" in lib.gca_last_error()


def test_varlen_attention_refuses_what_varlen_qkvpacked_refuses():
    from gaussiancity_amd.attention import varlen_attention as f
    cu = torch.tensor([0, 8], dtype=torch.int32)
    for dtype in (torch.float16, torch.float32):
        qkv = torch.zeros(8, 3, 2, 16, dtype=dtype)
        with pytest.raises(TypeError, match="tensors"):
            f(qkv.numpy(), cu, 8)
        with pytest.raises(TypeError, match="int32"):
            f(qkv, cu.long(), 8)
        with pytest.raises(ValueError):
            f(qkv[:, :, 0], cu, 8)                                      # rank 3
        with pytest.raises(ValueError):
            f(qkv[:, :2], cu, 8)                                        # middle dimension 2
        with pytest.raises(ValueError, match="1-D"):
            f(qkv, cu[None], 8)
        with pytest.raises(ValueError, match="16, 32, 64"):
            f(torch.zeros(8, 3, 2, 24, dtype=dtype), cu, 8)
        with pytest.raises(ValueError, match="at least one head"):
            f(torch.zeros(8, 3, 0, 16, dtype=dtype), cu, 8)
        with pytest.raises(ValueError, match="max_seqlen"):
            f(qkv, cu, -1)
        with pytest.raises(TypeError, match="GPU"):
            f(qkv, cu, 8)                                               # CPU tensors: there is no CPU path
    with pytest.raises(TypeError, match="bfloat16"):
        f(torch.zeros(8, 3, 2, 16, dtype=torch.bfloat16), cu, 8)
    with pytest.raises(TypeError, match="float64"):
        f(torch.zeros(8, 3, 2, 16, dtype=torch.float64), cu, 8)
    from gaussiancity_amd.attention import varlen_qkvpacked
    with pytest.raises(TypeError, match="float16"):
        varlen_qkvpacked(torch.zeros(8, 3, 2, 16), cu, 8)              # the binary16 function still refuses float32


@pytest.mark.parametrize("i", range(len(R32.INPUT_SET)))
def test_emulated_float32_contract_within_eight_units(i):
    """8 units = 2 x the 3.7 measured for the contract in numpy float32 over this input set; guards the helper."""
    name, qkv, cu, dout, cut, ref = R32.input_case(i)
    worst = R32.errors_in_units(R32.emulate32(qkv, cu, dout, None, cut), ref)
    print(name, "Smax %.1f" % ref["smax"], worst)
    assert max(worst.values()) <= 8.0, (name, worst)
    assert all((ref["u_" + n] > 0).any() for n in R32.NAMES)


# ---- the backbone binding on a stand-in for models/pt_v3.py -----------------------------------------------------------
class _Point(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _stand_in():
    class SerializedAttention(torch.nn.Module):
        def __init__(self, enable_flash=False, enable_rpe=False, attn_drop=0.0):
            super().__init__()
            self.channels, self.num_heads, self.scale, self.order_index = 32, 2, 0.25, 0
            self.enable_flash, self.enable_rpe = enable_flash, enable_rpe
            self.patch_size_max, self.patch_size = 16, 0
            self.attn_drop = torch.nn.Dropout(attn_drop)
            self.qkv, self.proj, self.proj_drop = torch.nn.Linear(32, 96), torch.nn.Linear(32, 32), torch.nn.Dropout(0.0)
            self.calls = 0

        def get_padding_and_inverse(self, point):
            raise AssertionError("the fused path must not start on these inputs")

        def forward(self, point):
            self.calls += 1
            return "original"

    return types.SimpleNamespace(SerializedAttention=SerializedAttention, Point=_Point)


def test_point_attention_rebinds_restores_and_hands_the_rest_to_the_original():
    from gaussiancity_amd import point_attention as PA
    M = _stand_in()
    own = M.SerializedAttention.forward
    PA.install(M)
    rebound = M.SerializedAttention.forward
    assert rebound is not own
    PA.install(M)                                                       # idempotent: the original is not lost
    assert M.SerializedAttention.forward is rebound
    PA.reset_stats()
    assert PA.stats() == {"fused_calls": 0, "original_calls": 0}
    point = _Point(feat=torch.zeros(16, 32), offset=torch.tensor([16]))
    cases = [M.SerializedAttention(), M.SerializedAttention(enable_flash=True), M.SerializedAttention(enable_rpe=True),
             M.SerializedAttention(attn_drop=0.1)]
    for n, att in enumerate(cases, 1):                                  # CPU tensors, flash, RPE, active dropout
        assert att(point) == "original" and att.calls == 1
        assert PA.stats() == {"fused_calls": 0, "original_calls": n}
        assert att.patch_size == 0                                      # nothing of the fused path ran
    PA.uninstall(M)
    assert M.SerializedAttention.forward is own
    PA.uninstall(M)                                                     # idempotent
    assert M.SerializedAttention.forward is own
    assert cases[0](point) == "original" and PA.stats()["original_calls"] == 4   # the module's own method: not counted
    PA.reset_stats()
    assert PA.stats() == {"fused_calls": 0, "original_calls": 0}


def test_point_attention_is_independent_of_point_index():
    from gaussiancity_amd import point_attention as PA
    from gaussiancity_amd import point_index as PI
    M = _stand_in()
    M.Point.serialization = lambda self, **kw: None
    own = (M.SerializedAttention.forward, M.SerializedAttention.get_padding_and_inverse, M.Point.serialization)
    PA.install(M)
    PI.install(M)
    PA.uninstall(M)                                                     # either order, either alone
    assert M.SerializedAttention.forward is own[0] and M.SerializedAttention.get_padding_and_inverse is not own[1]
    PA.install(M)
    PI.uninstall(M)
    assert M.SerializedAttention.get_padding_and_inverse is own[1] and M.Point.serialization is own[2]
    assert M.SerializedAttention.forward is not own[0]
    PA.uninstall(M)
    assert M.SerializedAttention.forward is own[0]
