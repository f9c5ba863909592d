"""-m gpu: the split feed-forward entry points of libgcm_hip.so (gcm_ffn_split_*) through
gaussiancity_amd.ffn.layernorm_mlp_residual(..., split=True).

Bits.  Where the one-launch kernels run too (C <= 128) every output and the stored a / mean / rstd are theirs bit for bit,
through Python and through the C ABI over NaN-filled outputs and workspace; no tolerance is involved.  At the new widths:
two runs and two backwards over one graph, strided rows, dropped rows, gradient subsets, the no_grad forward and N = 0, as
tests/test_ffn_gpu.py holds them for the narrow operator.

Values at the new widths.  The bar of tests/ffn_ref.py: per tensor max|got - x64| / max|x64|, worst over the cases of one
(C, Hd), at most FACTOR x the same figure of the torch float32 ops on the same GPU against the float64 CPU run, never below
FLOOR.  Operator, yardstick and ratio are printed per tensor.

Modes.  The smallest N the plan puts in rows mode at (132, 528) -- found through the plan query, never stated here -- meets
the bar, and its first 64 rows have the y and dx of a run on those 64 rows alone (split mode)."""
import functools

import pytest
import torch

from ffn_ref import (EPS, FACTOR, FLOOR, LEAVES, TENSORS, bits, figures, make_inputs, run, same_bits,
                     torch_ops)
from ffn_ref import fused as narrow

pytestmark = pytest.mark.gpu
NS = (1, 63, 64, 65, 257)
NARROW = ((4, 4), (32, 128), (48, 40), (128, 512))       # both operators run
WIDE = ((132, 528), (256, 1024), (512, 2048), (388, 200))  # beyond the old cap; the last between instantiations, a partial chunk
PLUMBING = ((256, 1024), (512, 2048))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def split(t, s):
    from gaussiancity_amd.ffn import layernorm_mlp_residual
    return layernorm_mlp_residual(t["x"], t["ln_w"], t["ln_b"], EPS, t["w1"], t["b1"], t["w2"], t["b2"], s, split=True)


def scales(N):
    s = torch.tensor([0.0, 1.0, 1.0 / 0.7])[torch.randint(0, 3, (N,), generator=torch.Generator().manual_seed(N))]
    s[0] = 0.0
    if N > 1:
        s[1] = 1.0 / 0.7
    if N > 2:
        s[2] = 1.0
    return s


def special_rows(inp):
    """tests/test_ffn_gpu.py's: a constant row (variance 0) and a row scaled by 1e3 beside one scaled by 1e-3."""
    x = inp["x"].clone()
    x[3] = 2.5
    x[10] *= 1e3
    x[11] *= 1e-3
    return dict(inp, x=x)


@functools.lru_cache(maxsize=None)
def target(N, C, Hd, seed, kind):
    """(inputs, row_scale, the float64 CPU run): computed once, shared, never changed."""
    inp = make_inputs(N, C, Hd, seed)
    s = None
    if kind == "scale":
        s = scales(N)
    elif kind == "special":
        inp = special_rows(inp)
    return inp, s, run(torch_ops, inp, "cpu", torch.float64, s)


def check_bar(label, cases, dev):
    """ffn_ref.check_bar for the split operator; cases: (inputs, row_scale, float64 run) that share one (C, Hd)."""
    worst_got, worst_yard = dict.fromkeys(TENSORS, 0.0), dict.fromkeys(TENSORS, 0.0)
    for inp, s, want in cases:
        got = figures(run(split, inp, dev, torch.float32, s), want)
        yard = figures(run(torch_ops, inp, dev, torch.float32, s), want)
        for k in TENSORS:
            worst_got[k], worst_yard[k] = max(worst_got[k], got[k]), max(worst_yard[k], yard[k])
    failed = []
    for k in TENSORS:
        bar = max(FACTOR * worst_yard[k], FLOOR)
        print("%s %-5s operator %.3e  torch float32 %.3e  ratio %.2f  bar %.3e" % (
            label, k, worst_got[k], worst_yard[k], worst_got[k] / max(worst_yard[k], 1e-30), bar))
        if not worst_got[k] <= bar:
            failed.append((k, worst_got[k], bar))
    assert not failed, failed


# ---- 1. the bits of the one-launch operator where both run -------------------------------------------------------------
@pytest.mark.parametrize("C,Hd", NARROW)
def test_split_gives_the_bits_of_the_one_launch_operator(dev, C, Hd):
    from gaussiancity_amd import ffn
    for N in NS:
        inp, s = make_inputs(N, C, Hd, 1000 + N), scales(N)
        before = ffn.split_stats()
        got = run(split, inp, dev, torch.float32, s)
        assert ffn.split_stats() == {"forward_calls": before["forward_calls"] + 1, "backward_calls": before["backward_calls"] + 1}
        assert same_bits(got, run(narrow, inp, dev, torch.float32, s)), (C, Hd, N)
        assert same_bits(run(split, inp, dev, torch.float32), run(narrow, inp, dev, torch.float32)), (C, Hd, N)


def abi_run(lib, M, d, s, N, C, Hd, dev, which):
    """One forward and one backward through the C ABI over NaN-filled outputs (and, for the split entry points, workspaces):
    y, the seven gradients and the stored a / mean / rstd."""
    import ctypes
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)  # noqa: E731
    p = lambda k: d[k].data_ptr()  # noqa: E731
    sp = None if s is None else s.data_ptr()
    y, mean, rstd, a = nan(N, C), nan(N), nan(N), nan(N, Hd)
    out = {"dx": nan(N, C), "dln_w": nan(C), "dln_b": nan(C), "dw1": nan(Hd, C), "db1": nan(Hd), "dw2": nan(C, Hd), "db2": nan(C)}
    fwd_args = (p("x"), C, p("ln_w"), p("ln_b"), EPS, p("w1"), p("b1"), p("w2"), p("b2"), sp, N, C, Hd, y.data_ptr(), C,
                mean.data_ptr(), rstd.data_ptr(), a.data_ptr())
    if which == "split":
        fb, bb = ctypes.c_size_t(), ctypes.c_size_t()
        M.check(lib.gcm_ffn_split_workspace_bytes(N, C, Hd, ctypes.byref(fb), ctypes.byref(bb)), "bytes")
        wf, need = nan(fb.value // 4), bb.value
        M.check(lib.gcm_ffn_split_forward(*fwd_args, wf.data_ptr(), fb.value, None), "forward")
        backward = lib.gcm_ffn_split_backward
    else:
        need = lib.gcm_ffn_backward_workspace_bytes(N, C, Hd)
        M.check(lib.gcm_ffn_forward(*fwd_args, None), "forward")
        backward = lib.gcm_ffn_backward
    ws = nan(need // 4)
    M.check(backward(p("x"), C, mean.data_ptr(), rstd.data_ptr(), a.data_ptr(), p("dy"), C, sp, p("ln_w"), p("ln_b"), p("w1"),
                     p("w2"), N, C, Hd, out["dx"].data_ptr(), C, out["dln_w"].data_ptr(), out["dln_b"].data_ptr(),
                     out["dw1"].data_ptr(), out["db1"].data_ptr(), out["dw2"].data_ptr(), out["db2"].data_ptr(),
                     ws.data_ptr(), need, None), "backward")
    torch.cuda.synchronize()
    out.update(y=y, mean=mean, rstd=rstd, a=a)
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("C,Hd", NARROW)
def test_through_the_c_abi_over_nan_the_stored_tensors_and_every_output_have_the_same_bits(dev, C, Hd):
    from gaussiancity_amd import _native_m as M
    lib = M.lib()
    for N in NS:
        inp = make_inputs(N, C, Hd, 1100 + N)
        d = {k: v.to(dev) for k, v in inp.items()}
        s = scales(N).to(dev)
        one, two = abi_run(lib, M, d, s, N, C, Hd, dev, "narrow"), abi_run(lib, M, d, s, N, C, Hd, dev, "split")
        for k in one:
            assert bool(torch.isfinite(two[k]).all()), (k, N)
            assert torch.equal(bits(one[k]), bits(two[k])), (k, C, Hd, N)


# ---- 2. the bar at the new widths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,Hd", WIDE)
def test_every_output_at_the_new_widths_is_within_four_times_torchs_own_float32_error(dev, C, Hd):
    check_bar("C=%d Hd=%d" % (C, Hd), [target(N, C, Hd, 100 + N, "plain") for N in NS], dev)


@pytest.mark.parametrize("C,Hd", WIDE)
def test_row_scale_meets_the_bar_at_the_new_widths(dev, C, Hd):
    check_bar("row_scale C=%d Hd=%d" % (C, Hd), [target(N, C, Hd, 200 + N, "scale") for N in NS], dev)


@pytest.mark.parametrize("C,Hd", WIDE)
def test_a_constant_row_and_rows_of_very_different_scale_meet_the_bar_at_the_new_widths(dev, C, Hd):
    check_bar("special rows C=%d Hd=%d" % (C, Hd), [target(65, C, Hd, 300, "special")], dev)


# ---- 3. both modes, and rows that do not know their N -----------------------------------------------------------------------
def test_rows_mode_meets_the_bar_and_its_first_tile_has_the_bits_of_a_run_on_that_tile_alone(dev):
    from gaussiancity_amd import ffn
    C, Hd = 132, 528
    limit = ffn.split_plan(257, C, Hd)["limit"]
    chunks = ffn.split_plan(257, C, Hd)["chunks"]
    N = 64 * (limit // chunks) + 1                       # the first tile count beyond the limit ...
    assert ffn.split_plan(N, C, Hd)["mode"] == "rows" and ffn.split_plan(N - 1, C, Hd)["mode"] == "split"  # ... says the query
    assert ffn.split_plan(257, C, Hd)["mode"] == "split" and ffn.split_plan(N, C, Hd)["records"] == 1
    inp, s, want = target(N, C, Hd, 1300, "scale")
    check_bar("rows mode N=%d C=%d Hd=%d" % (N, C, Hd), [(inp, s, want)], dev)
    big = run(split, inp, dev, torch.float32, s)
    head = {k: (v[:64] if k in ("x", "dy") else v) for k, v in inp.items()}
    small = run(split, head, dev, torch.float32, s[:64])
    assert ffn.split_plan(64, C, Hd)["mode"] == "split"
    assert torch.equal(bits(big["y"][:64]), bits(small["y"])) and torch.equal(bits(big["dx"][:64]), bits(small["dx"]))


# ---- 4. determinism and plumbing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,Hd", PLUMBING)
def test_two_runs_and_two_backwards_over_one_graph_are_bit_identical(dev, C, Hd):
    inp = make_inputs(257, C, Hd, 500)
    s = torch.rand(257, generator=torch.Generator().manual_seed(5))
    assert same_bits(run(split, inp, dev, torch.float32, s), run(split, inp, dev, torch.float32, s))
    t = {k: inp[k].to(dev).requires_grad_(True) for k in LEAVES}
    y = split(t, s.to(dev))
    y.backward(inp["dy"].to(dev), retain_graph=True)
    first = {k: t[k].grad.clone() for k in t}
    for k in t:
        t[k].grad = None
    y.backward(inp["dy"].to(dev))      # the saved pre-activation was read, not overwritten
    assert all(torch.equal(bits(first[k]), bits(t[k].grad)) for k in t)


@pytest.mark.parametrize("C,Hd", PLUMBING)
def test_strided_rows_give_the_bits_of_their_contiguous_copies(dev, C, Hd):
    for N in (65, 257):
        inp = make_inputs(N, C, Hd, 400 + N)
        assert same_bits(run(split, inp, dev, torch.float32), run(split, inp, dev, torch.float32, stride=C + 8))


@pytest.mark.parametrize("C,Hd", PLUMBING)
def test_a_dropped_row_is_the_shortcut_bit_for_bit(dev, C, Hd):
    for N in (65, 257):
        inp, s = make_inputs(N, C, Hd, 200 + N), scales(N)
        s[N - 1] = 0.0
        got = run(split, inp, dev, torch.float32, s)
        dropped = s == 0
        assert int(dropped.sum()) >= 2
        assert torch.equal(bits(got["y"][dropped]), bits(inp["x"][dropped]))
        assert torch.equal(bits(got["dx"][dropped]), bits(inp["dy"][dropped]))


@pytest.mark.parametrize("C,Hd", PLUMBING)
def test_outputs_and_workspace_prefilled_with_nan_come_back_fully_written(dev, C, Hd):
    from gaussiancity_amd import _native_m as M
    N = 130
    inp = make_inputs(N, C, Hd, 600)
    want = run(split, inp, dev, torch.float32)
    got = abi_run(M.lib(), M, {k: v.to(dev) for k, v in inp.items()}, None, N, C, Hd, dev, "split")
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert same_bits(got, want)


@pytest.mark.parametrize("C,Hd", PLUMBING)
def test_each_single_gradient_and_each_complement_of_six_has_the_bits_of_the_all_seven_run(dev, C, Hd):
    inp, s = make_inputs(65, C, Hd, 1400), scales(65)
    full = run(split, inp, dev, torch.float32, s)
    name = lambda leaf: "dx" if leaf == "x" else "d" + leaf  # noqa: E731
    for leaf in LEAVES:
        for need in ((leaf,), tuple(k for k in LEAVES if k != leaf)):
            got = run(split, inp, dev, torch.float32, s, need=need)
            assert torch.equal(bits(got["y"]), bits(full["y"]))
            for k in LEAVES:
                if k in need:
                    assert torch.equal(bits(got[name(k)]), bits(full[name(k)])), (need, k)
                else:
                    assert got[name(k)] is None, (need, k)


@pytest.mark.parametrize("C,Hd", PLUMBING)
def test_the_inference_forward_gives_the_bits_of_the_grad_mode_forward_and_stores_nothing_else(dev, C, Hd):
    from gaussiancity_amd import ffn
    for N in (1, 65, 257):
        inp = make_inputs(N, C, Hd, 800 + N)
        t = {k: inp[k].to(dev) for k in LEAVES}
        before, before_split = ffn.stats(), ffn.split_stats()
        with torch.no_grad():
            y0 = split(t, None)
        y1 = split({k: v.clone().requires_grad_(True) for k, v in t.items()}, None)
        assert not y0.requires_grad and y0.grad_fn is None and y1.requires_grad
        assert torch.equal(bits(y0), bits(y1.detach()))
        assert ffn.stats()["forward_calls"] == before["forward_calls"] + 2
        assert ffn.split_stats()["forward_calls"] == before_split["forward_calls"] + 2


def test_no_rows_give_empty_tensors_and_zero_parameter_gradients(dev):
    C, Hd = 256, 1024
    got = run(split, make_inputs(0, C, Hd, 700), dev, torch.float32)
    assert got["y"].shape == (0, C) and got["dx"].shape == (0, C)
    assert all(got[k].shape == s and not got[k].any() for k, s in (("dw1", (Hd, C)), ("dw2", (C, Hd)), ("db1", (Hd,)),
                                                                  ("db2", (C,)), ("dln_w", (C,)), ("dln_b", (C,))))


def test_the_default_path_still_refuses_a_width_beyond_its_cap_and_split_names_its_own(dev):
    from gaussiancity_amd import ffn
    w = {k: v.to(dev) for k, v in make_inputs(5, 132, 16, 901).items()}
    with pytest.raises(ValueError, match="the fused kernels hold"):
        ffn.layernorm_mlp_residual(w["x"], w["ln_w"], w["ln_b"], EPS, w["w1"], w["b1"], w["w2"], w["b2"])
    w = {k: v.to(dev) for k, v in make_inputs(5, 516, 16, 902).items()}
    with pytest.raises(ValueError, match="the fused kernels hold C up to 512"):
        ffn.layernorm_mlp_residual(w["x"], w["ln_w"], w["ln_b"], EPS, w["w1"], w["b1"], w["w2"], w["b2"], split=True)
