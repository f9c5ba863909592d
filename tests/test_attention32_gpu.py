"""-m gpu: the float32 attention (attention.varlen_attention -> the `_t` entry points of include/gca.h -> the gfx950
kernels on v_mfma_f32_16x16x4_f32) and its binding to the PTv3 backbone (gaussiancity_amd.point_attention).

Units (tests/attn_ref32.py): one float32 unit of an element is 2^-24 (1 + Smax) A.  Over the input set of attn_ref32, per
tensor of out, dQ, dK, dV, the kernels' worst error in units must stay within 2 x the worst of the backbone's own float32
formulation (torch, same GPU, same run).  Both evaluate the same formulas in fp32; they differ in summation order (the
MFMA's k order, key blocks with rescaling), in the exponential (v_exp_f32 against torch's) and in P, which the backward
recomputes from the log-sum-exp.  A binary16 rounding anywhere would be about 2^13 / (1 + Smax) units, roughly 1000 at
Smax <= 6: the factor 2 cannot hide one.

Bit-exact where the rule is a copy (one-hot attention) or the same computation (strides, two runs, GCA_F16 through the
typed entry points), and the backbone binding against the reference's own float64 results (tests/golden)."""
import os

import numpy as np
import pytest
import torch

import attn_ref as R
import attn_ref32 as R32

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ptv3_attention.npz")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_a
    _native_a.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _run(dev, qkv, cu, dout, max_seqlen, scale=None):
    """Forward + backward through varlen_attention; out, dq, dk, dv as numpy arrays of qkv's dtype."""
    from gaussiancity_amd.attention import varlen_attention
    x = (qkv if isinstance(qkv, torch.Tensor) else torch.from_numpy(qkv).to(dev)).requires_grad_(True)
    out = varlen_attention(x, torch.from_numpy(np.asarray(cu, np.int32)).to(dev), max_seqlen, softmax_scale=scale)
    assert out.dtype == x.dtype and tuple(out.shape) == (x.shape[0], x.shape[2], x.shape[3])
    out.backward(dout if isinstance(dout, torch.Tensor) else torch.from_numpy(dout).to(dev))
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
    g = x.grad.cpu().numpy()
    return {"out": out.detach().cpu().numpy(), "dq": g[:, 0], "dk": g[:, 1], "dv": g[:, 2]}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- units ------------------------------------------------------------------------------------------------------------
def test_units_within_twice_the_torch_float32_formulation(dev):
    """Measured on an MI355X, worst float32 units over the input set, kernels / torch float32: out 1.78 / 1.79,
    dQ 1.10 / 0.88, dK 0.93 / 1.07, dV 2.05 / 2.52 (DESIGN.md section 16 has what it took: the exact log-sum-exp and the
    two-level sums)."""
    kernel, yard = [], []
    for i in range(len(R32.INPUT_SET)):
        name, qkv, cu, dout, cut, ref = R32.input_case(i)
        max_seqlen = int(np.diff(cu).max()) if cut is None else cut
        k = R32.errors_in_units(_run(dev, qkv, cu, dout, max_seqlen), ref)
        t = R32.errors_in_units(R32.torch32(qkv, cu, dout, None, cut, device=dev), ref)
        print("%-24s Smax %6.1f  kernel %s  torch %s" % (name, ref["smax"], {n: round(v, 2) for n, v in k.items()},
                                                        {n: round(v, 2) for n, v in t.items()}))
        kernel.append(k)
        yard.append(t)
    kernel, yard = R32.worst_of(kernel), R32.worst_of(yard)
    for n in R32.NAMES:
        print("worst float32 units, %-3s: kernel %.2f, torch float32 %.2f, bar %.2f" % (n, kernel[n], yard[n], 2 * yard[n]))
    for n in R32.NAMES:
        assert kernel[n] <= 2 * yard[n], (n, kernel, yard)


# ---- bit-exact cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 32, 64])
def test_orientation_one_hot_is_a_copy(dev, d):
    # q_i = 30 e_((i + 1) mod len), k_j = 30 e_j, scale 0.25: the matching score is 225 above every other one, whose
    # exp is 0 in fp32.  The shift makes P asymmetric: a transposed operand, a swapped row / column map or a k slot of
    # the four-step product that reads another element of the fragment cannot pass.  Lengths up to d use every channel.
    lens, heads = [d, 5, 1, 9, d - 3, 2], 2
    qkv, cu, dout = R32.random_case32(61 + d, lens, heads, d)
    total = qkv.shape[0]
    src = np.zeros(total, np.int64)
    qkv[:, :2] = 0
    for b, n in R.segments(cu, total):
        for i in range(n):
            src[b + i] = b + (i + 1) % n
            qkv[b + i, 0, :, (i + 1) % n] = 30
            qkv[b + i, 1, :, i] = 30
    got = _run(dev, qkv, cu, dout, d, 0.25)
    assert _same_bits(got["out"], qkv[src, 2]), "out[i] is not v[(i + 1) mod len]"
    assert _same_bits(got["dv"][src], dout), "dV[(i + 1) mod len] is not dOut[i]"


def test_segments_do_not_leak(dev):
    qkv, cu, dout = R32.random_case32(71, [100, 60], heads=2)
    a = _run(dev, qkv, cu, dout, 128, 0.25)
    other = qkv.copy()
    other[100:, 1:] = R32.random_case32(72, [60], heads=2)[0][:, 1:] * np.float32(3)
    b = _run(dev, other, cu, dout, 128, 0.25)
    assert _same_bits(a["out"][:100], b["out"][:100]) and not _same_bits(a["out"][100:], b["out"][100:])
    for n in R.NAMES:
        assert _same_bits(a[n][:100], b[n][:100]), n


def test_rows_outside_every_segment_are_zero(dev):
    qkv, _, dout = R32.random_case32(73, [64], heads=2)
    got = _run(dev, qkv, [8, 40], dout, 64, 0.25)
    for n in R.NAMES:
        assert not got[n][:8].any() and not got[n][40:].any() and got[n][8:40].any(), n
    # out-of-range entries are clamped on the device, a decreasing pair is an empty segment
    got = _run(dev, qkv, [-5, 24, 1000, 8], dout, 64, 0.25)
    ref = R32.reference32(qkv, np.array([0, 24, 64, 64], np.int32), dout, 0.25)
    worst = R32.errors_in_units(got, ref)
    print("clamped cu_seqlens: float32 units", worst)
    assert max(worst.values()) <= 8.0                                  # attn_ref32's bar for a float32 evaluation
    # a segment longer than max_seqlen: the rows beyond max_seqlen are zeros
    got = _run(dev, qkv, [0, 64], dout, 16, 0.25)
    for n in R.NAMES:
        assert not got[n][16:].any() and got[n][:16].any(), n


def test_empty_inputs(dev):
    from gaussiancity_amd.attention import varlen_attention as f
    x = torch.zeros(0, 3, 2, 16, device=dev, requires_grad=True)
    out = f(x, torch.zeros(1, dtype=torch.int32, device=dev), 0)
    assert tuple(out.shape) == (0, 2, 16) and out.dtype == torch.float32
    out.sum().backward()
    assert tuple(x.grad.shape) == (0, 3, 2, 16)
    y = torch.ones(8, 3, 2, 16, device=dev, requires_grad=True)
    out = f(y, torch.zeros(1, dtype=torch.int32, device=dev), 8)          # no segment at all
    out.sum().backward()
    assert not out.any() and not y.grad.any()


@pytest.mark.parametrize("d", [16, 32, 64])
def test_strided_float32_qkv_gives_the_same_bits(dev, d):
    """A slice of a wider projection: the row stride and the offset are multiples of 4 elements, not of 8."""
    from gaussiancity_amd import attention as AT
    heads = 3
    qkv, cu, dout = R32.random_case32(500 + d, [200, 56, 300], heads=heads, d=d)
    total, width = qkv.shape[0], 3 * heads * d
    wide = torch.zeros(total, width + 20, device=dev)
    wide[:, 4:4 + width] = torch.from_numpy(qkv).to(dev).reshape(total, width)
    view = wide[:, 4:4 + width].view(total, 3, heads, d).detach()
    assert not view.is_contiguous() and view.stride() == (width + 20, heads * d, d, 1) and AT._kernel_ready(view)
    # dout as a slice of a wider row, too
    gwide = torch.full((total, heads * d + 12), 7.0, device=dev)
    gwide[:, 4:4 + heads * d] = torch.from_numpy(dout).to(dev).reshape(total, heads * d)
    gview = gwide[:, 4:4 + heads * d].view(total, heads, d)
    assert AT._kernel_ready(gview) and not gview.is_contiguous()
    a = _run(dev, view, cu, gview, 300, None)
    b = _run(dev, qkv, cu, dout, 300, None)
    for n in R.NAMES:
        assert _same_bits(a[n], b[n]), n
    # a row stride that is no multiple of 4 goes through a contiguous copy: same bits again
    odd = torch.zeros(total, width + 2, device=dev)
    odd[:, :width] = torch.from_numpy(qkv).to(dev).reshape(total, width)
    oview = odd[:, :width].view(total, 3, heads, d).detach()
    assert not AT._kernel_ready(oview)
    c = _run(dev, oview, cu, dout, 300, None)
    for n in R.NAMES:
        assert _same_bits(c[n], b[n]), n


def test_two_runs_are_bit_identical(dev):
    qkv, cu, dout = R32.random_case32(91, [1024, 700, 64, 333], 2)
    a = _run(dev, qkv, cu, dout, 1024, 0.25)
    b = _run(dev, qkv, cu, dout, 1024, 0.25)
    for n in R.NAMES:
        assert _same_bits(a[n], b[n]), n


@pytest.mark.parametrize("d", [16, 32, 64])
def test_f16_through_the_typed_entry_points_gives_the_bits_of_the_untyped_ones(dev, d):
    from gaussiancity_amd import _native_a as A
    from gaussiancity_amd.attention import varlen_qkvpacked
    heads, lens = 2, [130, 1, 0, 77, 200]
    qkv, cu, dout = R.random_case(800 + d, lens, heads, d)
    total = qkv.shape[0]
    x, g, c = torch.from_numpy(qkv).to(dev), torch.from_numpy(dout).to(dev), torch.from_numpy(cu).to(dev)
    L = A.lib()
    ws_bytes = L.gca_backward_workspace_bytes(total, heads)
    res = []
    for typed in (False, True):
        out = torch.full((total, heads, d), 7.0, dtype=torch.float16, device=dev)
        lse = torch.full((heads, total), 7.0, dtype=torch.float32, device=dev)
        dqkv = torch.full((total, 3, heads, d), 7.0, dtype=torch.float16, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        head = (0,) if typed else ()
        fwd = L.gca_varlen_forward_t if typed else L.gca_varlen_forward
        bwd = L.gca_varlen_backward_t if typed else L.gca_varlen_backward
        A.check(fwd(*head, x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), c.data_ptr(), len(lens), total, heads, d, 256,
                    0.25, out.data_ptr(), lse.data_ptr(), None), "forward")
        A.check(bwd(*head, x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), out.data_ptr(), g.data_ptr(), g.stride(0),
                    g.stride(1), lse.data_ptr(), c.data_ptr(), len(lens), total, heads, d, 256, 0.25, dqkv.data_ptr(),
                    ws.data_ptr(), ws_bytes, None), "backward")
        torch.cuda.synchronize()
        res.append((out.cpu().numpy(), lse.cpu().numpy(), dqkv.cpu().numpy()))
    for a, b in zip(*res):
        assert _same_bits(a, b)
    xg = x.clone().requires_grad_(True)
    o = varlen_qkvpacked(xg, c, 256, 0.25)
    o.backward(g)
    assert _same_bits(o.detach().cpu().numpy(), res[1][0]) and _same_bits(xg.grad.cpu().numpy(), res[1][2])


# ---- no score tensor --------------------------------------------------------------------------------------------------
def test_no_score_tensor_in_memory(dev):
    from gaussiancity_amd.attention import varlen_attention
    total, heads = 4096, 2
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(total, 3, heads, 16, device=dev, generator=gen).requires_grad_(True)
    cu = torch.arange(0, total + 1, 1024, dtype=torch.int32, device=dev)
    scores = 4 * heads * 1024 * 1024 * 4                                # one [4, 2, 1024, 1024] float32 tensor
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = varlen_attention(x, cu, 1024, softmax_scale=0.25)
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print("peak grew by %.2f MB; qkv is %.2f MB, one score tensor %.1f MB" % (grew / 1e6, x.numel() * 4 / 1e6, scores / 1e6))
    assert grew < scores
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x.grad).all())


# ---- the backbone binding against the reference's float64 results ------------------------------------------------------
class _Point(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _stand_in():
    """What install() needs of models/pt_v3.py, written for this test.  Every method of its own raises: whatever the
    test computes comes from the rebound ones."""
    import types

    class SerializedAttention(torch.nn.Module):
        def __init__(self, channels, num_heads, patch_size):
            super().__init__()
            self.channels, self.num_heads, self.scale, self.order_index = channels, num_heads, (channels // num_heads) ** -0.5, 0
            self.enable_flash = self.enable_rpe = False
            self.patch_size_max, self.patch_size = patch_size, 0
            self.attn_drop, self.proj_drop = torch.nn.Dropout(0.0), torch.nn.Dropout(0.0)
            self.qkv, self.proj = torch.nn.Linear(channels, channels * 3), torch.nn.Linear(channels, channels)

        def get_padding_and_inverse(self, point):
            raise AssertionError("the module's own get_padding_and_inverse ran")

        def forward(self, point):
            raise AssertionError("the module's own forward ran")

    class Point(_Point):
        def serialization(self, order="z", depth=None, shuffle_orders=False):
            raise AssertionError("the module's own serialization ran")

    return types.SimpleNamespace(SerializedAttention=SerializedAttention, Point=Point)


PARAMS = ("qkv.weight", "qkv.bias", "proj.weight", "proj.bias")


@pytest.fixture(scope="module")
def bound(dev):
    from gaussiancity_amd import point_attention as PA
    from gaussiancity_amd import point_index as PI
    M = _stand_in()
    PI.install(M)
    PA.install(M)
    yield M, np.load(GOLDEN)
    PA.uninstall(M)
    PI.uninstall(M)


def _backbone(dev, M, gold, case, autocast):
    att = M.SerializedAttention(32, 2, int(gold[case + ".patch"])).to(dev)
    with torch.no_grad():
        for name in PARAMS:
            att.get_parameter(name).copy_(torch.from_numpy(gold["%s.%s" % (case, name)]))
    feat = torch.from_numpy(gold[case + ".feat"]).to(dev).requires_grad_(True)
    point = M.Point(feat=feat, offset=torch.from_numpy(np.cumsum(gold[case + ".counts"])).to(dev),
                    serialized_order=torch.from_numpy(gold[case + ".order"]).to(dev),
                    serialized_inverse=torch.from_numpy(gold[case + ".inverse"]).to(dev))
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        out = att(point).feat
    (out.float() * torch.from_numpy(gold[case + ".w"]).to(dev)).sum().backward()
    res = {"out": out.detach(), "grad.feat": feat.grad}
    res.update({"grad." + name: att.get_parameter(name).grad for name in PARAMS})
    return att, {k: v.double().cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("case", ["k37", "k64", "k16"])
def test_backbone_binding_matches_the_reference_in_float32(dev, bound, case):
    """Per tensor within 4 x the error of the reference's own float32 run against its float64 run (the two Linears run
    in rocBLAS's summation order rather than the CPU's); binary16 anywhere would be about 1e-3, a thousand times above."""
    from gaussiancity_amd import point_attention as PA
    M, gold = bound
    before = PA.stats()
    att, got = _backbone(dev, M, gold, case, autocast=False)
    assert att.patch_size == int(gold[case + ".K"])
    assert PA.stats() == {"fused_calls": before["fused_calls"] + 1, "original_calls": before["original_calls"]}
    for name, x in got.items():
        x64 = gold["%s.%s" % (case, name)]
        err, bar = np.abs(x - x64).max() / np.abs(x64).max(), 4 * float(gold["%s.err32.%s" % (case, name)])
        print("%s %-16s %.2e of the maximum, bar %.2e" % (case, name, err, bar))
        assert err <= bar, (case, name, err, bar)


@pytest.mark.parametrize("case", ["k37", "k64", "k16"])
def test_backbone_binding_under_autocast_runs_the_binary16_kernels(dev, bound, case, monkeypatch):
    from gaussiancity_amd import point_attention as PA
    M, gold = bound
    seen = []
    inner = PA.attention.varlen_attention
    monkeypatch.setattr(PA.attention, "varlen_attention", lambda qkv, *a, **kw: (seen.append(qkv.dtype), inner(qkv, *a, **kw))[1])
    before = PA.stats()["fused_calls"]
    att, got = _backbone(dev, M, gold, case, autocast=True)
    assert seen == [torch.float16] and PA.stats()["fused_calls"] == before + 1
    assert att.patch_size == int(gold[case + ".K"])
    for name, x in got.items():
        x64 = gold["%s.%s" % (case, name)]
        err = np.abs(x - x64).max() / np.abs(x64).max()
        print("%s autocast %-16s %.2e of the maximum" % (case, name, err))
        assert err <= 5e-2, (case, name, err)
