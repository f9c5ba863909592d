"""CPU tests of the attention path (libgca_hip.so, include/gca.h; gaussiancity_amd.attention; the flash_attn
drop-in): the library loads (tests/test_cabi.py holds its exports to the header), the ABI rejects bad arguments before
it touches the device, the drop-in imports with upstream's signature and refuses what it does not implement, the
float64 reference (tests/attn_ref.py) agrees with torch, and the emulated rounding contract leaves the GPU bar its
headroom."""
import inspect

import numpy as np
import pytest
import torch

import attn_ref as R


@pytest.fixture(scope="module")
def lib():
    from gaussiancity_amd import _native_a as A
    return A.lib()


def test_size_queries(lib):
    assert lib.gca_lse_bytes(1000, 4) == 1000 * 4 * 4
    assert lib.gca_backward_workspace_bytes(262144, 2) == 262144 * 2 * 4      # O(total * H): delta only
    assert lib.gca_lse_bytes(-1, 4) == 0 and b"total" in lib.gca_last_error()
    assert lib.gca_backward_workspace_bytes(10, 0) == 0 and b"heads" in lib.gca_last_error()
    assert lib.gca_lse_bytes(0, 4) == 0 and lib.gca_last_error() == b""


def _fwd(lib, qkv=16, rs=96, ss=32, hs=16, cu=16, nseg=2, total=64, heads=2, d=16, max_seqlen=32, scale=0.25, out=16, lse=16):
    return lib.gca_varlen_forward(qkv, rs, ss, hs, cu, nseg, total, heads, d, max_seqlen, scale, out, lse, None)


def _bwd(lib, qkv=16, rs=96, ss=32, hs=16, out=16, dout=16, drs=32, dhs=16, lse=16, cu=16, nseg=2, total=64, heads=2, d=16,
         max_seqlen=32, scale=0.25, dqkv=16, ws=16, ws_bytes=64 * 2 * 4):
    return lib.gca_varlen_backward(qkv, rs, ss, hs, out, dout, drs, dhs, lse, cu, nseg, total, heads, d, max_seqlen, scale,
                                   dqkv, ws, ws_bytes, None)


def test_forward_rejects_bad_arguments_before_touching_the_device(lib):
    # dummy non-null, 16-byte aligned device addresses: every call below must fail in the argument checks
    assert _fwd(lib, qkv=None) < 0 and b"null" in lib.gca_last_error()
    assert _fwd(lib, out=None) < 0 and b"null" in lib.gca_last_error()
    assert _fwd(lib, lse=None) < 0
    assert _fwd(lib, cu=None) < 0 and b"cu_seqlens" in lib.gca_last_error()
    assert _fwd(lib, heads=0) < 0 and b"heads" in lib.gca_last_error()
    assert _fwd(lib, heads=-3) < 0
    for d in (0, 8, 24, 48, 128):
        assert _fwd(lib, d=d) < 0 and b"head_dim must be 16, 32 or 64" in lib.gca_last_error()
    assert _fwd(lib, total=-1) < 0 and b"total" in lib.gca_last_error()
    assert _fwd(lib, max_seqlen=-1) < 0 and b"max_seqlen" in lib.gca_last_error()
    assert _fwd(lib, nseg=-1) < 0 and b"nseg" in lib.gca_last_error()
    assert _fwd(lib, rs=0) < 0 and b"strides" in lib.gca_last_error()
    assert _fwd(lib, hs=12) < 0 and b"strides" in lib.gca_last_error()
    assert _fwd(lib, qkv=8) < 0 and b"aligned" in lib.gca_last_error()
    assert _fwd(lib, scale=float("nan")) < 0 and b"softmax_scale" in lib.gca_last_error()
    assert _fwd(lib, nseg=2 ** 30, max_seqlen=2 ** 20, total=2 ** 30) < 0 and b"grid" in lib.gca_last_error()
    assert _fwd(lib, total=0, qkv=None, out=None, lse=None, cu=None) == 0      # an empty problem is no error


def test_backward_rejects_bad_arguments_before_touching_the_device(lib):
    for name in ("qkv", "out", "dout", "lse", "dqkv"):
        assert _bwd(lib, **{name: None}) < 0 and b"null" in lib.gca_last_error(), name
    assert _bwd(lib, cu=None) < 0 and b"cu_seqlens" in lib.gca_last_error()
    assert _bwd(lib, heads=0) < 0 and b"heads" in lib.gca_last_error()
    assert _bwd(lib, d=20) < 0 and b"head_dim" in lib.gca_last_error()
    assert _bwd(lib, total=-5) < 0 and b"total" in lib.gca_last_error()
    assert _bwd(lib, max_seqlen=-1) < 0 and b"max_seqlen" in lib.gca_last_error()
    assert _bwd(lib, drs=4) < 0 and b"strides" in lib.gca_last_error()
    assert _bwd(lib, dout=4) < 0 and b"aligned" in lib.gca_last_error()
    assert _bwd(lib, ws=None) < 0 and b"workspace" in lib.gca_last_error()
    need = lib.gca_backward_workspace_bytes(64, 2)
    assert _bwd(lib, ws_bytes=need - 1) < 0 and b"workspace" in lib.gca_last_error()
    assert _bwd(lib, total=0, qkv=None, dqkv=None, ws=None, ws_bytes=0) == 0


def test_drop_in_imports_with_upstreams_signature():
    import flash_attn
    import flash_attn.flash_attn_interface as FI
    from gaussiancity_amd import attention as AT
    assert flash_attn.flash_attn_varlen_qkvpacked_func is FI.flash_attn_varlen_qkvpacked_func
    assert isinstance(flash_attn.__version__, str) and flash_attn.__version__
    sig = inspect.signature(flash_attn.flash_attn_varlen_qkvpacked_func)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("qkv", inspect.Parameter.empty), ("cu_seqlens", inspect.Parameter.empty), ("max_seqlen", inspect.Parameter.empty),
        ("dropout_p", 0.0), ("softmax_scale", None), ("causal", False), ("window_size", (-1, -1)), ("softcap", 0.0),
        ("alibi_slopes", None), ("deterministic", False), ("return_attn_probs", False)]
    assert 16 in AT.SUPPORTED_HEAD_DIMS
    assert all(d % 16 == 0 and d <= 64 for d in AT.SUPPORTED_HEAD_DIMS)


def test_refusals_of_the_python_layer_without_a_gpu():
    from flash_attn import flash_attn_varlen_qkvpacked_func as f
    qkv = torch.zeros(8, 3, 2, 16, dtype=torch.float16)
    cu = torch.tensor([0, 8], dtype=torch.int32)
    for kw, word in (({"dropout_p": 0.1}, "dropout_p"), ({"causal": True}, "causal"), ({"window_size": (4, 4)}, "window_size"),
                     ({"window_size": (-1, 0)}, "window_size"), ({"softcap": 1.0}, "softcap"),
                     ({"alibi_slopes": torch.zeros(2)}, "alibi_slopes"), ({"return_attn_probs": True}, "return_attn_probs")):
        with pytest.raises(NotImplementedError, match=word):
            f(qkv, cu, 8, **kw)
    with pytest.raises(TypeError, match="float16"):
        f(qkv.to(torch.bfloat16), cu, 8)
    with pytest.raises(TypeError, match="float16"):
        f(qkv.float(), cu, 8)
    with pytest.raises(TypeError, match="int32"):
        f(qkv, cu.long(), 8)
    with pytest.raises(ValueError):
        f(qkv[:, :, 0], cu, 8)                                        # rank 3
    with pytest.raises(ValueError):
        f(torch.zeros(8, 2, 2, 16, dtype=torch.float16), cu, 8)       # middle dimension 2
    with pytest.raises(ValueError, match="16, 32, 64"):
        f(torch.zeros(8, 3, 2, 24, dtype=torch.float16), cu, 8)       # head dimension not offered: names the supported ones
    with pytest.raises(ValueError, match="16, 32, 64"):
        f(torch.zeros(8, 3, 2, 128, dtype=torch.float16), cu, 8)
    with pytest.raises(TypeError, match="GPU"):
        f(qkv, cu, 8, deterministic=True)                              # accepted argument, CPU tensors refused


def _torch_segment(q, k, v, do, scale):
    t = [torch.from_numpy(np.ascontiguousarray(a)).double().requires_grad_(True) for a in (q, k, v)]
    out = torch.nn.functional.scaled_dot_product_attention(t[0][None], t[1][None], t[2][None], scale=scale)[0]
    out.backward(torch.from_numpy(np.ascontiguousarray(do)).double())
    return [out.detach().numpy()] + [a.grad.numpy() for a in t]


@pytest.mark.parametrize("scale", [None, 0.5])
def test_reference_agrees_with_torch_float64(scale):
    lens = [1, 7, 0, 33, 16]
    qkv, cu, dout = R.random_case(11, lens, heads=2)
    ref = R.reference(qkv, cu, dout, scale)
    s = 16 ** -0.5 if scale is None else scale
    x, g = qkv.astype(np.float64), dout.astype(np.float64)
    for b, n in R.segments(cu, qkv.shape[0]):
        for h in range(2):
            if n == 0:
                continue
            want = _torch_segment(x[b:b + n, 0, h], x[b:b + n, 1, h], x[b:b + n, 2, h], g[b:b + n, h], s)
            for name, w in zip(R.NAMES, want):
                got = ref[name][b:b + n, h]
                assert np.abs(got - w).max() <= 1e-12 * max(np.abs(w).max(), 1e-300), (name, b, h)
    assert all((ref["u_" + n] > 0).all() for n in R.NAMES)


def test_reference_leaves_uncovered_rows_zero():
    qkv, _, dout = R.random_case(3, [64], heads=1)
    cu = np.array([8, 40], np.int32)
    ref = R.reference(qkv, cu, dout, 0.25)
    for n in R.NAMES:
        assert not ref[n][:8].any() and not ref[n][40:].any() and ref[n][8:40].any()
    got = {n: ref[n].copy() for n in R.NAMES}
    assert max(R.errors_in_units(got, ref).values()) == 0
    got["dq"][3, 0, 0] = 1e-9
    assert R.errors_in_units(got, ref)["dq"] == np.inf                  # nothing is left out of the comparison
    ref2 = R.reference(qkv, np.array([0, 64], np.int32), dout, 0.25, max_seqlen=16)
    assert not ref2["out"][16:].any() and ref2["out"][:16].any()


def _emulated_worst(qkv, cu, dout, scale, max_seqlen=None):
    return R.errors_in_units(R.emulate(qkv, cu, dout, scale, max_seqlen), R.reference(qkv, cu, dout, scale, max_seqlen))


def test_emulated_contract_within_two_units_ragged():
    for seed, scale in ((21, 0.25), (22, None), (23, 0.5)):
        qkv, cu, dout = R.random_case(seed, R.RAGGED_LENS, heads=3)
        worst = _emulated_worst(qkv, cu, dout, scale)
        print("ragged scale", scale, worst)
        assert max(worst.values()) <= 2.0, (scale, worst)


@pytest.mark.parametrize("v_amp,do_amp", [(1.0, 1.0), (5.0, 0.01)])
def test_emulated_contract_within_two_units_amplitude(v_amp, do_amp):
    for i, amp in enumerate(R.AMPLITUDES):
        qkv, cu, dout = R.random_case(40 + i, [1024], heads=1, qk_amp=amp, v_amp=v_amp, do_amp=do_amp)
        worst = _emulated_worst(qkv, cu, dout, 0.25)
        print("amplitude", amp, v_amp, do_amp, worst)
        assert max(worst.values()) <= 2.0, (amp, worst)


# ---- the twins of the cases that tests/test_varlen_attention_gpu.py adds at head dimensions 32 and 64: the same seeds,
# lengths, scales and cuts; the rounding contract alone must leave the GPU bar (4 units) half of its room
SWEEP_LENS = R.RAGGED_LENS + [127, 128, 129, 191, 192, 193, 257]


@pytest.mark.parametrize("d,scale", [(d, s) for d in (16, 32, 64) for s in (None, 0.25)] + [(64, -0.25), (64, 0.0)])
def test_emulated_contract_within_two_units_length_sweep(d, scale):
    qkv, cu, dout = R.random_case(200 + d, SWEEP_LENS, heads=3, d=d)
    got = R.emulate(qkv, cu, dout, scale)
    worst = R.errors_in_units(got, R.reference(qkv, cu, dout, scale))
    print("length sweep", d, scale, worst)
    assert max(worst.values()) <= 2.0, (d, scale, worst)
    if scale == 0.0:
        assert not got["dq"].any() and not got["dk"].any()


@pytest.mark.parametrize("amp", [1.0, 3.0, 6.0])
@pytest.mark.parametrize("d", [32, 64])
def test_emulated_contract_within_two_units_amplitude_other_head_dims(d, amp):
    qkv, cu, dout = R.random_case(300 + d + int(amp), [300], heads=1, d=d, qk_amp=amp)
    worst = _emulated_worst(qkv, cu, dout, None)
    print("amplitude", d, amp, worst)
    assert max(worst.values()) <= 2.0, (d, amp, worst)


@pytest.mark.parametrize("d,cut", [(32, 100), (64, 65)])
def test_emulated_contract_within_two_units_cut_by_max_seqlen(d, cut):
    qkv, cu, dout = R.random_case(400 + d, [300, 70], heads=2, d=d)
    worst = _emulated_worst(qkv, cu, dout, None, cut)
    print("cut", d, cut, worst)
    assert max(worst.values()) <= 2.0, (d, cut, worst)
    ref = R.reference(qkv, cu, dout, None, cut)
    assert not ref["u_out"][cut:300].any() and ref["u_out"][:cut].all() and not ref["out"][300 + min(cut, 70):].any()


@pytest.mark.parametrize("d", [32, 64])
def test_emulated_contract_within_two_units_strided_twin(d):
    qkv, cu, dout = R.random_case(500 + d, [200, 56, 300], heads=3, d=d)
    worst = _emulated_worst(qkv, cu, dout, None)
    print("strided twin", d, worst)
    assert max(worst.values()) <= 2.0, (d, worst)


@pytest.mark.parametrize("d", [16, 32, 64])
def test_emulated_contract_within_two_units_dout_layouts(d):
    """The random dout of the layout cases, its float32 variant rounded to binary16, and dout = 1 (out.sum().backward())."""
    qkv, cu, dout = R.random_case(600 + d, [130, 1, 0, 77, 200], heads=3, d=d)
    d32 = np.random.default_rng(d).normal(size=dout.shape).astype(np.float32)
    for what, g in (("random", dout), ("rounded float32", d32.astype(np.float16)), ("ones", np.ones_like(dout))):
        worst = _emulated_worst(qkv, cu, g, None, 256)
        print("dout", what, d, worst)
        assert max(worst.values()) <= 2.0, (d, what, worst)


@pytest.mark.parametrize("d", [16, 32, 64])
def test_emulated_contract_within_two_units_lse_case(d):
    lens = [1, 2, 63, 64, 65, 129, 300, 0, 5]
    qkv, cu, dout = R.random_case(700 + d, lens, heads=2, d=d, total=sum(lens) + 9)
    worst = _emulated_worst(qkv, cu, dout, None, 1024)
    print("lse case", d, worst)
    assert max(worst.values()) <= 2.0, (d, worst)
