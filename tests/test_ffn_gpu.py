"""-m gpu: the feed-forward operator of libgcm_hip.so through gaussiancity_amd.ffn.layernorm_mlp_residual.

Values.  The target is the same formulation in float64 on the CPU from the same float32 inputs; the yardstick is the torch
float32 formulation (F.layer_norm, F.linear, F.gelu, F.linear, add) on the same GPU in the same run.  Per (C, Hd) and per
tensor (y, dx and the six parameter gradients) the figure max|got - x64| / max|x64|, worst over the N values, is at most
4 x the yardstick's same figure -- the project's factor for another summation order (tests/test_attr_head_gpu.py) -- and
the bar is never held below 2^-23, two float32 roundings of the largest element.  Both figures are printed per tensor.

Bits.  Rows with row_scale 0 have y == x and dx == dy; strided x / dy give the bits of their contiguous copies; two runs
(and two backwards over one retained graph) give the same bits; outputs and workspace pre-filled with NaN come back fully
written; N = 0 gives empty tensors; the no_grad forward (hidden tensor never stored) gives the grad-mode y.

Inputs, the two formulations, the runner and the bar are in tests/ffn_ref.py, shared with tests/test_ffn_plans_gpu.py."""
import pytest
import torch

from ffn_ref import (EPS, PARAMS, bits, check_bar, figures, fused, make_inputs, run, same_bits,  # noqa: F401
                     torch_ops)

pytestmark = pytest.mark.gpu
NS = (1, 63, 64, 65, 257)                               # the row-tile edges, more than one tile
SHAPES = ((4, 4), (32, 128), (48, 40), (128, 512))      # a hidden width that is no whole chunk, the widest required tile


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def special_rows(inp):
    """A constant row (variance 0) and a row scaled by 1e3 beside one scaled by 1e-3."""
    x = inp["x"].clone()
    x[3] = 2.5
    x[10] *= 1e3
    x[11] *= 1e-3
    return dict(inp, x=x)


@pytest.mark.parametrize("C,Hd", SHAPES)
def test_every_output_is_within_four_times_torchs_own_float32_error(dev, C, Hd):
    check_bar("C=%d Hd=%d" % (C, Hd), [(make_inputs(N, C, Hd, 100 + N), None) for N in NS], dev)


@pytest.mark.parametrize("C,Hd", SHAPES)
def test_row_scale_meets_the_bar_and_a_dropped_row_is_the_shortcut_bit_for_bit(dev, C, Hd):
    cases = []
    for N in (65, 257):
        inp = make_inputs(N, C, Hd, 200 + N)
        s = torch.tensor([0.0, 1.0, 1.0 / 0.7])[torch.randint(0, 3, (N,), generator=torch.Generator().manual_seed(N))]
        s[0], s[1], s[N - 1] = 0.0, 1.0 / 0.7, 0.0
        cases.append((inp, s))
        got = run(fused, inp, dev, torch.float32, s)
        dropped = s == 0
        assert int(dropped.sum()) >= 2
        assert torch.equal(bits(got["y"][dropped]), bits(inp["x"][dropped]))
        assert torch.equal(bits(got["dx"][dropped]), bits(inp["dy"][dropped]))
    check_bar("row_scale C=%d Hd=%d" % (C, Hd), cases, dev)


@pytest.mark.parametrize("C,Hd", SHAPES)
def test_a_constant_row_and_rows_of_very_different_scale_meet_the_bar(dev, C, Hd):
    check_bar("special rows C=%d Hd=%d" % (C, Hd), [(special_rows(make_inputs(65, C, Hd, 300)), None)], dev)


@pytest.mark.parametrize("C,Hd", SHAPES)
def test_strided_rows_give_the_bits_of_their_contiguous_copies(dev, C, Hd):
    for N in (65, 257):
        inp = make_inputs(N, C, Hd, 400 + N)
        assert same_bits(run(fused, inp, dev, torch.float32), run(fused, inp, dev, torch.float32, stride=C + 8))


@pytest.mark.parametrize("C,Hd", SHAPES)
def test_two_runs_and_two_backwards_over_one_graph_are_bit_identical(dev, C, Hd):
    inp = make_inputs(257, C, Hd, 500)
    s = torch.rand(257, generator=torch.Generator().manual_seed(5))
    assert same_bits(run(fused, inp, dev, torch.float32, s), run(fused, inp, dev, torch.float32, s))
    t = {k: inp[k].to(dev).requires_grad_(True) for k in ("x",) + PARAMS}
    y = fused(t, s.to(dev))
    y.backward(inp["dy"].to(dev), retain_graph=True)
    first = {k: t[k].grad.clone() for k in t}
    for k in t:
        t[k].grad = None
    y.backward(inp["dy"].to(dev))      # the saved pre-activation was read, not overwritten
    assert all(torch.equal(bits(first[k]), bits(t[k].grad)) for k in t)


@pytest.mark.parametrize("C,Hd", SHAPES)
def test_outputs_and_workspace_prefilled_with_nan_come_back_fully_written(dev, C, Hd):
    from gaussiancity_amd import _native_m as M
    lib, N = M.lib(), 130
    inp = make_inputs(N, C, Hd, 600)
    want = run(fused, inp, dev, torch.float32)
    d = {k: v.to(dev) for k, v in inp.items()}
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)  # noqa: E731
    y, mean, rstd, a = nan(N, C), nan(N), nan(N), nan(N, Hd)
    p = lambda k: d[k].data_ptr()  # noqa: E731
    M.check(lib.gcm_ffn_forward(p("x"), C, p("ln_w"), p("ln_b"), EPS, p("w1"), p("b1"), p("w2"), p("b2"), None, N, C, Hd,
                                y.data_ptr(), C, mean.data_ptr(), rstd.data_ptr(), a.data_ptr(), None), "forward")
    out = {"dx": nan(N, C), "dln_w": nan(C), "dln_b": nan(C), "dw1": nan(Hd, C), "db1": nan(Hd), "dw2": nan(C, Hd), "db2": nan(C)}
    need = lib.gcm_ffn_backward_workspace_bytes(N, C, Hd)
    ws = nan(need // 4 + 1)
    M.check(lib.gcm_ffn_backward(p("x"), C, mean.data_ptr(), rstd.data_ptr(), a.data_ptr(), p("dy"), C, None, p("ln_w"),
                                 p("ln_b"), p("w1"), p("w2"), N, C, Hd, out["dx"].data_ptr(), C, out["dln_w"].data_ptr(),
                                 out["dln_b"].data_ptr(), out["dw1"].data_ptr(), out["db1"].data_ptr(),
                                 out["dw2"].data_ptr(), out["db2"].data_ptr(), ws.data_ptr(), need, None), "backward")
    torch.cuda.synchronize()
    out["y"] = y
    for k in ("mean", "rstd", "a"):
        assert bool(torch.isfinite({"mean": mean, "rstd": rstd, "a": a}[k]).all()), k
    assert same_bits({k: v.cpu() for k, v in out.items()}, want)


def test_no_rows_give_empty_tensors_and_zero_parameter_gradients(dev):
    got = run(fused, make_inputs(0, 32, 128, 700), dev, torch.float32)
    assert got["y"].shape == (0, 32) and got["dx"].shape == (0, 32)
    assert all(got[k].shape == s and not got[k].any() for k, s in (("dw1", (128, 32)), ("dw2", (32, 128)), ("db1", (128,)),
                                                                  ("db2", (32,)), ("dln_w", (32,)), ("dln_b", (32,))))


@pytest.mark.parametrize("C,Hd", SHAPES)
def test_the_inference_forward_gives_the_bits_of_the_grad_mode_forward(dev, C, Hd):
    from gaussiancity_amd import ffn
    for N in (1, 65, 257):
        inp = make_inputs(N, C, Hd, 800 + N)
        t = {k: inp[k].to(dev) for k in ("x",) + PARAMS}
        before = ffn.stats()
        with torch.no_grad():
            y0 = fused(t, None)
        y1 = fused({k: v.clone().requires_grad_(True) for k, v in t.items()}, None)
        assert not y0.requires_grad and y1.requires_grad and torch.equal(bits(y0), bits(y1.detach()))
        assert ffn.stats()["forward_calls"] == before["forward_calls"] + 2


def test_bad_shapes_are_named(dev):
    from gaussiancity_amd import ffn
    t = {k: v.to(dev) for k, v in make_inputs(5, 8, 16, 900).items()}
    with pytest.raises(ValueError, match="ln_weight must be"):
        ffn.layernorm_mlp_residual(t["x"], torch.ones(12, device=dev), t["ln_b"], EPS, t["w1"], t["b1"], t["w2"], t["b2"])
    with pytest.raises(ValueError, match="row_scale must be"):
        ffn.layernorm_mlp_residual(t["x"], t["ln_w"], t["ln_b"], EPS, t["w1"], t["b1"], t["w2"], t["b2"], torch.ones(4, device=dev))
    wide = ffn.max_channels() + 4
    w = {k: v.to(dev) for k, v in make_inputs(5, wide, 16, 901).items()}
    with pytest.raises(ValueError, match="the fused kernels hold"):
        ffn.layernorm_mlp_residual(w["x"], w["ln_w"], w["ln_b"], EPS, w["w1"], w["b1"], w["w2"], w["b2"])
