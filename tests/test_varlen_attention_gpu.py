"""-m gpu: the flash_attn drop-in (flash_attn/ -> gaussiancity_amd.attention -> include/gca.h -> gfx950 MFMA
kernels) against the float64 reference tests/attn_ref.py.

Bar: every element of out, dQ, dK, dV within 4 UNITS of the float64 value, one unit = 2^-11 * (the formula with
absolute values) + the subnormal floor (attn_ref's docstring).  2 units is the derived bound for out and dV (two
roundings to binary16: the operand P and the stored result), dQ and dK add the rounding of dS and of the stored out
inside D; 4 leaves room for fp32 summation order and the hardware exponential.  Bit-exact where the rule is a copy
(one-hot attention), bit-identical between two runs (no float atomics)."""
import numpy as np
import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu
BAR = 4.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_a
    _native_a.lib()
    yield torch.device("cuda:0")
    # hand the cached blocks back: the 262 144-row case holds hundreds of MB
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _run(dev, qkv, cu, dout, max_seqlen, scale=None):
    """Forward + backward through the drop-in; out, dq, dk, dv as numpy binary16.  `dout` is a numpy array (copied to the
    device, contiguous), a tensor that is handed to backward() as it is, or None for out.sum().backward()."""
    import flash_attn
    x = (qkv if isinstance(qkv, torch.Tensor) else torch.from_numpy(qkv).to(dev)).requires_grad_(True)
    out = flash_attn.flash_attn_varlen_qkvpacked_func(x, torch.from_numpy(np.asarray(cu, np.int32)).to(dev), max_seqlen,
                                                      softmax_scale=scale)
    assert out.dtype == torch.float16 and tuple(out.shape) == (x.shape[0], x.shape[2], x.shape[3])
    if dout is None:
        out.sum().backward()
    else:
        out.backward(dout if isinstance(dout, torch.Tensor) else torch.from_numpy(dout).to(dev))
    assert x.grad.dtype == torch.float16 and x.grad.shape == x.shape
    g = x.grad.cpu().numpy()
    return {"out": out.detach().cpu().numpy(), "dq": g[:, 0], "dk": g[:, 1], "dv": g[:, 2]}


def _check(dev, qkv, cu, dout, max_seqlen, scale, what, bar=BAR):
    got = _run(dev, qkv, cu, dout, max_seqlen, scale)
    worst = R.errors_in_units(got, R.reference(qkv, cu, dout, scale, max_seqlen))
    print("%s: worst error in units %s" % (what, {k: round(v, 3) for k, v in worst.items()}))
    assert all(v <= bar for v in worst.values()), (what, worst)
    return got


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint16), np.asarray(b).view(np.uint16))


PTV3_STAGES = [(16384, 2, [1024] * 16), (5120, 4, [1024] * 5), (2048, 8, [1024] * 2), (271, 16, [271]), (73, 32, [73])]


@pytest.mark.parametrize("rows,heads,lens", PTV3_STAGES, ids=["stage%d" % i for i in range(5)])
def test_ptv3_stages(dev, rows, heads, lens):
    qkv, cu, dout = R.random_case(100 + heads, lens, heads)
    assert qkv.shape[0] == rows
    _check(dev, qkv, cu, dout, 1024, 0.25, "PTv3 %d rows x %d heads" % (rows, heads))


@pytest.mark.parametrize("scale", [0.25, None, 0.5])
def test_ragged(dev, scale):
    qkv, cu, dout = R.random_case(21, R.RAGGED_LENS, heads=3)
    _check(dev, qkv, cu, dout, 1024, scale, "ragged, scale %r" % (scale,))


def test_long_segment(dev):
    qkv, cu, dout = R.random_case(31, [4096], heads=2)
    _check(dev, qkv, cu, dout, 4096, None, "one segment of 4096")


@pytest.mark.parametrize("v_amp,do_amp", [(1.0, 1.0), (5.0, 0.01)])
@pytest.mark.parametrize("amp", R.AMPLITUDES)
def test_amplitude(dev, amp, v_amp, do_amp):
    qkv, cu, dout = R.random_case(40 + R.AMPLITUDES.index(amp), [1024], heads=1, qk_amp=amp, v_amp=v_amp, do_amp=do_amp)
    _check(dev, qkv, cu, dout, 1024, 0.25, "amplitude %g, V x %g, dOut x %g" % (amp, v_amp, do_amp))


@pytest.mark.parametrize("d", [32, 64])
def test_other_head_dims(dev, d):
    from gaussiancity_amd.attention import SUPPORTED_HEAD_DIMS
    assert d in SUPPORTED_HEAD_DIMS
    qkv, cu, dout = R.random_case(50 + d, [1, 17, 64, 130, 300, 0, 77], heads=2, d=d)
    _check(dev, qkv, cu, dout, 300, None, "head dimension %d" % d)


SWEEP_LENS = R.RAGGED_LENS + [127, 128, 129, 191, 192, 193, 257]


@pytest.mark.parametrize("d,scale", [(d, s) for d in (16, 32, 64) for s in (None, 0.25)] + [(64, -0.25), (64, 0.0)])
def test_length_sweep_at_every_head_dim(dev, d, scale):
    """Every staged-block boundary (64-key steps, 128-row blocks, the 64-row blocks of the dK/dV pass at d = 64) at every
    head dimension: the LDS pitches differ with d."""
    qkv, cu, dout = R.random_case(200 + d, SWEEP_LENS, heads=3, d=d)
    got = _check(dev, qkv, cu, dout, 1024, scale, "length sweep d = %d, scale %r" % (d, scale))
    if scale == 0.0:
        # uniform attention: the reference that _check compared with IS the segment's mean of V, and scale * dS is exactly zero
        assert not got["dq"].any() and not got["dk"].any()
        ref = R.reference(qkv, cu, dout, scale)["out"]
        v = qkv[:, 2].astype(np.float64)
        for b, n in R.segments(cu, qkv.shape[0]):
            if n:
                assert np.abs(ref[b:b + n] - v[b:b + n].mean(axis=0)).max() <= 1e-12


@pytest.mark.parametrize("amp", [1.0, 3.0, 6.0])
@pytest.mark.parametrize("d", [32, 64])
def test_amplitude_at_other_head_dims(dev, d, amp):
    qkv, cu, dout = R.random_case(300 + d + int(amp), [300], heads=1, d=d, qk_amp=amp)
    _check(dev, qkv, cu, dout, 300, None, "d = %d, amplitude %g" % (d, amp))


@pytest.mark.parametrize("d,cut", [(32, 100), (64, 65)])
def test_cut_by_max_seqlen_against_the_reference(dev, d, cut):
    """A segment longer than max_seqlen is its first max_seqlen rows: those match the reference of the cut segment, the
    rows beyond have unit 0 and must be exact zeros (errors_in_units counts anything else as infinitely wrong)."""
    qkv, cu, dout = R.random_case(400 + d, [300, 70], heads=2, d=d)
    got = _run(dev, qkv, cu, dout, cut, None)
    ref = R.reference(qkv, cu, dout, None, max_seqlen=cut)
    worst = R.errors_in_units(got, ref)
    print("cut at %d, d = %d: worst error in units %s" % (cut, d, {k: round(v, 3) for k, v in worst.items()}))
    assert all(v <= BAR for v in worst.values()), worst
    kept = min(cut, 70)                                     # of the second segment, rows 300 .. 369
    for n in R.NAMES:
        assert ref["u_" + n][:cut].all() and not ref["u_" + n][cut:300].any() and not ref["u_" + n][300 + kept:].any()
        assert got[n][:cut].any() and not got[n][cut:300].any(), n
        assert got[n][300:300 + kept].any() and not got[n][300 + kept:].any(), n


def test_orientation_one_hot_is_a_copy(dev):
    # q_i = 30 e_((i + 1) mod len), k_j = 30 e_j, scale 0.25: the matching score is 225 above every other one, whose
    # exp is 0 in fp32.  The shift makes P asymmetric: a transposed operand or a swapped row / column map cannot pass.
    lens, heads = [16, 5, 1, 9, 12, 2], 2
    qkv, cu, dout = R.random_case(61, lens, heads)
    total = qkv.shape[0]
    src = np.zeros(total, np.int64)
    qkv[:, :2] = 0
    for b, n in R.segments(cu, total):
        for i in range(n):
            src[b + i] = b + (i + 1) % n
            qkv[b + i, 0, :, (i + 1) % n] = 30
            qkv[b + i, 1, :, i] = 30
    got = _run(dev, qkv, cu, dout, 16, 0.25)
    assert _same_bits(got["out"], qkv[src, 2]), "out[i] is not v[(i + 1) mod len]"
    assert _same_bits(got["dv"][src], dout), "dV[(i + 1) mod len] is not dOut[i]"


def test_orientation_uniform_attention_is_the_mean(dev):
    qkv, cu, dout = R.random_case(62, [16, 5, 1, 100, 64, 37], heads=2)
    qkv[:, :2] = 0
    got = _check(dev, qkv, cu, dout, 128, 0.25, "Q = K = 0", bar=1.0)
    v = qkv[:, 2].astype(np.float64)
    for b, n in R.segments(cu, qkv.shape[0]):
        assert np.abs(got["out"][b:b + n] - v[b:b + n].mean(axis=0)).max() <= 2e-3


def test_segments_do_not_leak(dev):
    qkv, cu, dout = R.random_case(71, [100, 60], heads=2)
    a = _run(dev, qkv, cu, dout, 128, 0.25)
    other = qkv.copy()
    other[100:, 1:] = R.random_case(72, [60], heads=2)[0][:, 1:] * np.float16(3)
    b = _run(dev, other, cu, dout, 128, 0.25)
    assert _same_bits(a["out"][:100], b["out"][:100]) and not _same_bits(a["out"][100:], b["out"][100:])
    for n in ("dq", "dk", "dv"):
        assert _same_bits(a[n][:100], b[n][:100]), n


def test_rows_outside_every_segment_are_zero(dev):
    qkv, _, dout = R.random_case(73, [64], heads=2)
    got = _check(dev, qkv, [8, 40], dout, 64, 0.25, "cu_seqlens [8, 40] of 64 rows")
    for n in R.NAMES:
        assert not got[n][:8].any() and not got[n][40:].any() and got[n][8:40].any(), n
    # out-of-range entries are clamped on the device, a decreasing pair is an empty segment
    got = _run(dev, qkv, [-5, 24, 1000, 8], dout, 64, 0.25)
    ref = R.reference(qkv, [0, 24, 64, 64], dout, 0.25)
    assert max(R.errors_in_units(got, ref).values()) <= BAR
    # a segment longer than max_seqlen: the rows beyond max_seqlen are zeros
    got = _run(dev, qkv, [0, 64], dout, 16, 0.25)
    for n in R.NAMES:
        assert not got[n][16:].any() and got[n][:16].any(), n


def test_empty_inputs(dev):
    import flash_attn
    f = flash_attn.flash_attn_varlen_qkvpacked_func
    x = torch.zeros(0, 3, 2, 16, dtype=torch.float16, device=dev, requires_grad=True)
    out = f(x, torch.zeros(1, dtype=torch.int32, device=dev), 0)
    assert tuple(out.shape) == (0, 2, 16)
    out.sum().backward()
    assert tuple(x.grad.shape) == (0, 3, 2, 16)
    y = torch.ones(8, 3, 2, 16, dtype=torch.float16, device=dev, requires_grad=True)
    out = f(y, torch.zeros(1, dtype=torch.int32, device=dev), 8)          # no segment at all
    out.sum().backward()
    assert not out.any() and not y.grad.any()


def test_strided_qkv_gives_the_same_bits(dev):
    qkv, cu, dout = R.random_case(81, [200, 56, 1024], heads=4)
    total, width = qkv.shape[0], 3 * 4 * 16
    wide = torch.zeros(total, width + 64, dtype=torch.float16, device=dev)
    wide[:, 8:8 + width] = torch.from_numpy(qkv).to(dev).reshape(total, width)
    view = wide[:, 8:8 + width].view(total, 3, 4, 16).detach()
    assert not view.is_contiguous() and view.stride(0) == width + 64
    a = _run(dev, view, cu, dout, 1024, 0.25)
    b = _run(dev, qkv, cu, dout, 1024, 0.25)
    for n in R.NAMES:
        assert _same_bits(a[n], b[n]), n
    # [3, total, H, d] storage (slot stride above the row stride) still goes through the strides; [total, 3, d, H]
    # storage (no unit stride along d) goes through a contiguous copy: same bits again
    for dims in ((1, 0, 2, 3), (0, 1, 3, 2)):
        perm = torch.from_numpy(qkv).to(dev).permute(*dims).contiguous().permute(*dims).detach()
        assert not perm.is_contiguous() and perm.shape == view.shape
        c = _run(dev, perm, cu, dout, 1024, 0.25)
        for n in R.NAMES:
            assert _same_bits(c[n], b[n]), (dims, n)


@pytest.mark.parametrize("d", [32, 64])
def test_strided_qkv_gives_the_same_bits_at_other_head_dims(dev, d):
    heads = 3
    qkv, cu, dout = R.random_case(500 + d, [200, 56, 300], heads=heads, d=d)
    total, width = qkv.shape[0], 3 * heads * d
    wide = torch.zeros(total, width + 64, dtype=torch.float16, device=dev)
    wide[:, 8:8 + width] = torch.from_numpy(qkv).to(dev).reshape(total, width)
    view = wide[:, 8:8 + width].view(total, 3, heads, d).detach()
    assert not view.is_contiguous() and view.stride() == (width + 64, heads * d, d, 1)
    a = _run(dev, view, cu, dout, 300, None)
    b = _check(dev, qkv, cu, dout, 300, None, "contiguous twin of the strided view, d = %d" % d)
    for n in R.NAMES:
        assert _same_bits(a[n], b[n]), n


@pytest.mark.parametrize("d", [16, 32, 64])
def test_strided_and_converted_dout(dev, d):
    """dout_row_stride and dout_head_stride reach three kernels (delta, dK/dV, dQ); every layout that the autograd
    layer passes through as it is, and every one it converts, gives the bits of the contiguous binary16 dout."""
    heads = 3
    qkv, cu, dout = R.random_case(600 + d, [130, 1, 0, 77, 200], heads=heads, d=d)
    total = qkv.shape[0]
    base = _check(dev, qkv, cu, dout, 256, None, "contiguous dout, d = %d" % d)
    t = torch.from_numpy(dout).to(dev)
    # a slice of a wider row: the head stride is d, the row stride is not H * d
    wide = torch.full((total, heads * d + 64), 7.0, dtype=torch.float16, device=dev)
    wide[:, 8:8 + heads * d] = t.reshape(total, heads * d)
    row_view = wide[:, 8:8 + heads * d].view(total, heads, d)
    assert row_view.stride() == (heads * d + 64, d, 1)
    # the middle of a [total, H, 2 d] buffer: the head stride is larger than d
    deep = torch.full((total, heads, 2 * d), 7.0, dtype=torch.float16, device=dev)
    deep[:, :, 8:8 + d] = t
    head_view = deep[:, :, 8:8 + d]
    assert head_view.stride() == (2 * heads * d, 2 * d, 1)
    for what, g in (("row-strided", row_view), ("head-strided", head_view), ("float32", t.float())):
        got = _run(dev, qkv, cu, g, 256, None)
        for n in R.NAMES:
            assert _same_bits(got[n], base[n]), (what, n)
    # float32 values that are no binary16 numbers: the bits of their binary16 rounding
    rng = np.random.default_rng(d)
    d32 = rng.normal(size=dout.shape).astype(np.float32)
    got = _run(dev, qkv, cu, torch.from_numpy(d32).to(dev), 256, None)
    want = _run(dev, qkv, cu, d32.astype(np.float16), 256, None)
    for n in R.NAMES:
        assert _same_bits(got[n], want[n]), ("float32 rounding", n)
    # out.sum().backward(): an expanded dout (every stride 0) over real segments
    got = _run(dev, qkv, cu, None, 256, None)
    worst = R.errors_in_units(got, R.reference(qkv, cu, np.ones_like(dout), None, 256))
    print("expanded dout = 1, d = %d: worst error in units %s" % (d, {k: round(v, 3) for k, v in worst.items()}))
    assert all(v <= BAR for v in worst.values()), worst


@pytest.mark.parametrize("d", [16, 32, 64])
def test_log_sum_exp(dev, d):
    """lse [heads][total] of gca_varlen_forward, called directly: the float64 log-sum-exp on covered rows, exactly 0 on
    the others.

    Tolerance, from what the kernel does.  lse = (m + log2f(l)) * ln 2, m the fp32 maximum of the scores in units of
    log2, l the fp32 sum of v_exp_f32(s - m).  An error ds_j of score j moves lse by p_j ds_j, so the scores count
    with their softmax weight: at most max |ds_j| over the keys that matter, whose scores are near the maximum and so
    no larger than |lse| + log(n).  A score is d exact products summed in fp32 (d - 1 roundings of partial sums that
    are of the size of the score times a few: about sqrt(d) / 2 half-ulps as a random walk, 2 ulp at d = 64) and one
    product with scale * log2(e) (1/2 ulp).  Then 1 ulp for every v_exp_f32, the sum of up to 300 terms of one sign as 4
    partial sums per lane and two lane exchanges (about sqrt(300 / 16) half-ulps relative to l, i.e. 2 * 2^-24
    absolute on lse), 1 ulp for log2f, 1/2 each for the sum and the product with ln 2.  Together below 6 ulp; the
    bound is 8 ulp of max(|lse|, 1), ulp = 2^-23, and the worst ratio is printed."""
    from gaussiancity_amd import _native_a as A
    heads, lens = 2, [1, 2, 63, 64, 65, 129, 300, 0, 5]
    qkv, cu, _ = R.random_case(700 + d, lens, heads=heads, d=d, total=sum(lens) + 9)     # nine rows that no segment covers
    total = qkv.shape[0]
    scale = d ** -0.5
    x = torch.from_numpy(qkv).to(dev)
    cut = torch.from_numpy(cu).to(dev)
    out = torch.empty(total, heads, d, dtype=torch.float16, device=dev)
    lse = torch.full((heads, total), 7.0, dtype=torch.float32, device=dev)
    A.check(A.lib().gca_varlen_forward(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), cut.data_ptr(), len(lens), total,
                                       heads, d, 1024, scale, out.data_ptr(), lse.data_ptr(), None), "gca_varlen_forward")
    torch.cuda.synchronize()
    got = lse.cpu().numpy().astype(np.float64)
    want = np.zeros((heads, total))
    f = qkv.astype(np.float64)
    for b, n in R.segments(cu, total):
        for h in range(heads):
            if n:
                s = scale * (f[b:b + n, 0, h] @ f[b:b + n, 1, h].T)
                m = s.max(axis=1)
                want[h, b:b + n] = m + np.log(np.exp(s - m[:, None]).sum(axis=1))
    covered = np.zeros(total, bool)
    covered[:sum(lens)] = True
    assert not got[:, ~covered].any() and (~covered).sum() == 9
    tol = 8 * 2.0 ** -23 * np.maximum(np.abs(want), 1.0)
    err = np.abs(got - want)
    print("lse d = %d: worst error %.3g of the tolerance" % (d, float((err / tol)[:, covered].max())))
    assert (err <= tol)[:, covered].all()


def test_two_runs_are_bit_identical(dev):
    rows, heads, lens = PTV3_STAGES[0]
    qkv, cu, dout = R.random_case(91, lens, heads)
    a = _run(dev, qkv, cu, dout, 1024, 0.25)
    b = _run(dev, qkv, cu, dout, 1024, 0.25)
    for n in R.NAMES:
        assert _same_bits(a[n], b[n]), n


def test_no_score_tensor_in_memory(dev):
    import flash_attn
    total, heads = 262144, 2
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(total, 3, heads, 16, device=dev, generator=g).half().requires_grad_(True)
    cu = torch.arange(0, total + 1, 1024, dtype=torch.int32, device=dev)
    qkv_bytes = x.numel() * 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = flash_attn.flash_attn_varlen_qkvpacked_func(x, cu, 1024, softmax_scale=0.25)
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print("peak grew by %.1f MB = %.2f x qkv (%.1f MB)" % (grew / 1e6, grew / qkv_bytes, qkv_bytes / 1e6))
    assert grew < 4 * qkv_bytes
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x.grad).all())


class _Block(torch.nn.Module):
    """The calling pattern of PTv3's SerializedAttention, written for this test: qkv projection, gather by a padded
    order, attention over patches, inverse gather, output projection."""

    def __init__(self, channels, heads):
        super().__init__()
        self.heads, self.channels = heads, channels
        self.qkv = torch.nn.Linear(channels, 3 * channels)
        self.proj = torch.nn.Linear(channels, channels)

    def forward(self, feat, order, inverse, attend):
        qkv = self.qkv(feat)[order]
        out = attend(qkv.half().reshape(-1, 3, self.heads, self.channels // self.heads)).reshape(-1, self.channels)
        return self.proj(out.to(torch.float32)[inverse])


def test_as_ptv3_calls_it(dev):
    import flash_attn
    C, H, K, rows, n = 64, 4, 1024, 5120, 5000
    d, scale = C // H, (C // H) ** -0.5
    torch.manual_seed(7)
    block = _Block(C, H).to(dev)
    rng = np.random.default_rng(7)
    perm = rng.permutation(n)
    order_np = np.concatenate([perm, perm[n - K:n - K + (rows - n)]])       # the last patch borrows from the one before
    inverse_np = np.empty(n, np.int64)
    inverse_np[order_np[::-1]] = np.arange(rows)[::-1]                      # the first position that holds the point
    order, inverse = torch.from_numpy(order_np).to(dev), torch.from_numpy(inverse_np).to(dev)
    assert bool((order[inverse] == torch.arange(n, device=dev)).all())
    feat = torch.from_numpy(rng.normal(size=(n, C)).astype(np.float32)).to(dev)
    target = torch.from_numpy(rng.normal(size=(n, C)).astype(np.float32)).to(dev)
    cu = torch.arange(0, rows + 1, K, dtype=torch.int32, device=dev)

    def drop_in(x):
        return flash_attn.flash_attn_varlen_qkvpacked_func(x, cu, max_seqlen=K, dropout_p=0.0, softmax_scale=scale)

    def in_float64(x):
        q, k, v = x.double().reshape(-1, K, 3, H, d).permute(2, 0, 3, 1, 4)
        p = torch.softmax(scale * (q @ k.transpose(-1, -2)), dim=-1)
        return (p @ v).permute(0, 2, 1, 3).reshape(-1, H, d)

    def in_float16(x):
        q, k, v = x.reshape(-1, K, 3, H, d).permute(2, 0, 3, 1, 4)
        p = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
        assert p.dtype == torch.float16
        return (p @ v).permute(0, 2, 1, 3).reshape(-1, H, d)

    grads = []
    for attend in (drop_in, in_float64, in_float16):
        block.zero_grad(set_to_none=True)
        loss = (block(feat, order, inverse, attend) - target).square().sum()
        loss.backward()
        grads.append({k: p.grad.double().cpu().numpy() for k, p in block.named_parameters()})
    ours, ref, half = grads
    for name in ref:
        e_ours, e_half = np.abs(ours[name] - ref[name]).max(), np.abs(half[name] - ref[name]).max()
        print("%s: drop-in %.3e, float16 torch %.3e, max |ref| %.3e" % (name, e_ours, e_half, np.abs(ref[name]).max()))
        assert e_ours <= 3 * e_half + 1e-6 * np.abs(ref[name]).max(), name
