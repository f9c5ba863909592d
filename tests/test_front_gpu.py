"""-m gpu: the Block-front operator of libgcm_hip.so through gaussiancity_amd.front.conv_tail_norm_qkv.

Values.  The target is the formulation of tests/front_ref.py in float64 on the CPU from the same float32 inputs; the
yardstick is the torch float32 formulation (F.linear, F.layer_norm, add, F.layer_norm, F.linear) on the same GPU in the
same run.  Per (C, O) and per tensor (feat, qkv, dx, ds and the eight parameter gradients) the figure
max|got - x64| / max|x64|, worst over the N values, is at most 4 x the yardstick's same figure, and the bar is never held
below 2^-23.  Both figures are printed per tensor.  Plain inputs, the special rows of front_ref.special_rows, strided
x / s / dfeat / dqkv, the widths at which another kernel instantiation takes over, and the three large shapes of
tests/front_plans.py that reach the second fold level, the slice cap, slices without rows and chains longer than 32 rows.

Bits.  The inference forward (t == NULL) gives the training forward's feat and qkv; two runs give the same bits in every
output; outputs and workspace pre-filled with NaN come back fully written; every subset of the requested gradients gives
the bits of the all-outputs run; two backwards over one retained graph agree and leave the saved tensors as they were."""
import itertools

import pytest
import torch

import front_plans
from front_ref import (EPS_1, EPS_C, LEAVES, PARAMS, TENSORS, bits, check_bar, fused, make_inputs, run, same_bits,
                       special_rows)

pytestmark = pytest.mark.gpu
NS = (1, 63, 64, 65, 257)                               # the row-tile edges, more than one tile
SHAPES = ((4, 12), (32, 96), (48, 40), (128, 384))      # an O that is no whole chunk, the widest required tile
BOUNDARIES = ((36, 108), (68, 204), (100, 300), (128, 4), (128, 8))  # just past CT = 32 and 64, inside 128; O below a chunk


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("C,O", SHAPES)
def test_every_output_is_within_four_times_torchs_own_float32_error(dev, C, O):
    check_bar("C=%d O=%d" % (C, O), [make_inputs(N, C, O, 100 + N) for N in NS], dev)


@pytest.mark.parametrize("C,O", SHAPES)
def test_the_special_rows_meet_the_bar(dev, C, O):
    check_bar("special rows C=%d O=%d" % (C, O), [special_rows(make_inputs(N, C, O, 300 + N)) for N in NS if N >= 9], dev)


@pytest.mark.parametrize("C,O", SHAPES)
def test_strided_rows_meet_the_bar_and_give_the_bits_of_their_contiguous_copies(dev, C, O):
    cases = [make_inputs(N, C, O, 400 + N) for N in NS]
    check_bar("strided C=%d O=%d" % (C, O), cases, dev, strided=True)
    for inp in cases[2:]:
        assert same_bits(run(fused, inp, dev, torch.float32), run(fused, inp, dev, torch.float32, strided=True))


@pytest.mark.parametrize("C,O", BOUNDARIES)
def test_the_widths_at_which_another_instantiation_takes_over_meet_the_bar(dev, C, O):
    check_bar("boundary C=%d O=%d" % (C, O), [make_inputs(N, C, O, 500 + N) for N in (63, 130)], dev)


@pytest.mark.parametrize("N,C,O", sorted(front_plans.PLAN_CASES))
def test_the_large_plans_meet_the_bar(dev, N, C, O):
    """tests/test_front_host.py holds each shape to the branch it is here for."""
    check_bar("plan N=%d C=%d O=%d" % (N, C, O), [make_inputs(N, C, O, 600)], dev)


# ---- the C ABI directly: the buffers are the test's ------------------------------------------------------------------------
def _raw(dev, inp, prefill, training=True, outputs=TENSORS[2:]):
    """One forward and one backward through the library itself, every output and the workspace pre-filled."""
    from gaussiancity_amd import _native_m as M
    lib = M.lib()
    N, C = inp["x"].shape
    O = inp["wq"].shape[0]
    d = {k: v.to(dev) for k, v in inp.items()}
    p = lambda k: d[k].data_ptr()  # noqa: E731
    new = lambda *shape: torch.full(shape, prefill, device=dev)  # noqa: E731
    feat, qkv = new(N, C), new(N, O)
    t, st = (new(N, C), new(4, N)) if training else (None, None)
    sp = [None] * 4 if st is None else [st[k].data_ptr() for k in range(4)]
    M.check(lib.gcm_front_forward(p("x"), C, p("s"), C, p("wc"), p("bc"), p("gc"), p("bec"), EPS_C, p("g1"), p("be1"), EPS_1,
                                  p("wq"), p("bq"), N, C, O, feat.data_ptr(), C, qkv.data_ptr(), O,
                                  None if t is None else t.data_ptr(), *sp, None), "forward")
    out = {"feat": feat, "qkv": qkv}
    if training:
        shapes = {"dx": (N, C), "ds": (N, C), "dwc": (C, C), "dbc": (C,), "dgc": (C,), "dbec": (C,), "dg1": (C,), "dbe1": (C,),
                  "dwq": (O, C), "dbq": (O,)}
        g = {k: new(*shapes[k]) if k in outputs else None for k in shapes}
        q = lambda k: None if g[k] is None else g[k].data_ptr()  # noqa: E731
        need = lib.gcm_front_backward_workspace_bytes(N, C, O)
        ws = new(need // 4 + 1)
        M.check(lib.gcm_front_backward(p("s"), C, feat.data_ptr(), C, t.data_ptr(), *sp, p("dfeat"), C, p("dqkv"), O, p("wc"),
                                       p("gc"), p("g1"), p("be1"), p("wq"), N, C, O, q("dx"), C, q("ds"), C, q("dwc"), q("dbc"),
                                       q("dgc"), q("dbec"), q("dg1"), q("dbe1"), q("dwq"), q("dbq"), ws.data_ptr(), need, None),
                "backward")
        out.update({k: v for k, v in g.items() if v is not None}, t=t, stats=st)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("C,O", SHAPES)
def test_the_inference_forward_gives_the_bits_of_the_training_forward(dev, C, O):
    from gaussiancity_amd import front
    for N in (1, 65, 257):
        inp = make_inputs(N, C, O, 700 + N)
        a, b = _raw(dev, inp, float("nan"), training=False), _raw(dev, inp, float("nan"))
        assert same_bits(a, b, ("feat", "qkv")) and bool(torch.isfinite(b["t"]).all() and torch.isfinite(b["stats"]).all())
        t = {k: inp[k].to(dev) for k in LEAVES}
        before = front.stats()
        with torch.no_grad():
            f0, q0 = fused(t)
        f1, q1 = fused({k: v.clone().requires_grad_(True) for k, v in t.items()})
        assert not f0.requires_grad and f1.requires_grad and q1.requires_grad
        assert torch.equal(bits(f0), bits(f1.detach())) and torch.equal(bits(q0), bits(q1.detach()))
        assert torch.equal(bits(f0.cpu()), bits(a["feat"])) and torch.equal(bits(q0.cpu()), bits(a["qkv"]))
        assert front.stats()["forward_calls"] == before["forward_calls"] + 2


@pytest.mark.parametrize("N,C,O", [(257, C, O) for C, O in SHAPES] + [(4097, 4, 12), (4097, 128, 384)])
def test_two_runs_are_bit_identical(dev, N, C, O):
    inp = make_inputs(N, C, O, 800)
    assert same_bits(run(fused, inp, dev, torch.float32), run(fused, inp, dev, torch.float32))


@pytest.mark.parametrize("N,C,O", [(130, C, O) for C, O in SHAPES] + [(4097, 4, 12), (4097, 128, 384)])
def test_outputs_and_workspace_prefilled_with_nan_come_back_fully_written(dev, N, C, O):
    inp = make_inputs(N, C, O, 900)
    want = run(fused, inp, dev, torch.float32)
    a, b = _raw(dev, inp, float("nan")), _raw(dev, inp, 3.0)
    assert same_bits(a, want) and same_bits(b, want)
    assert torch.equal(bits(a["t"]), bits(b["t"])) and torch.equal(bits(a["stats"]), bits(b["stats"]))


def _subsets():
    singles = [(k,) for k in LEAVES]
    complements = [tuple(j for j in LEAVES if j != k) for k in LEAVES]
    return singles + complements


@pytest.mark.parametrize("C,O", SHAPES)
def test_single_gradients_and_their_complements_give_the_bits_of_the_all_outputs_run(dev, C, O):
    inp = make_inputs(130, C, O, 1000)
    full = run(fused, inp, dev, torch.float32)
    for need in _subsets():
        got = run(fused, inp, dev, torch.float32, need=need)
        for k in LEAVES:
            assert (got["d" + k] is None) == (k not in need), (need, k)
        assert same_bits(got, full, ("feat", "qkv") + tuple("d" + k for k in need)), need


def test_every_subset_of_the_outputs_gives_the_bits_of_the_all_outputs_run(dev):
    """All 1023 subsets at 130 x 48 x 40, through the library itself: a NULL output is skipped and changes no other."""
    inp = make_inputs(130, 48, 40, 1100)
    full = _raw(dev, inp, float("nan"))
    names = TENSORS[2:]
    for r in range(1, len(names)):
        for outputs in itertools.combinations(names, r):
            got = _raw(dev, inp, float("nan"), outputs=outputs)
            assert same_bits(got, full, ("feat", "qkv") + outputs), outputs


@pytest.mark.parametrize("C,O", SHAPES)
def test_two_backwards_over_one_graph_agree_and_leave_the_saved_tensors_alone(dev, C, O):
    inp = make_inputs(257, C, O, 1200)
    t = {k: inp[k].to(dev).requires_grad_(True) for k in LEAVES}
    feat, qkv = fused(t)
    saved = [v.clone() for v in feat.grad_fn.saved_tensors]
    grads = [inp["dfeat"].to(dev), inp["dqkv"].to(dev)]
    torch.autograd.backward([feat, qkv], grads, retain_graph=True)
    first = {k: t[k].grad.clone() for k in t}
    for k in t:
        t[k].grad = None
    again = feat.grad_fn.saved_tensors
    assert len(saved) == len(again) and all(torch.equal(bits(a), bits(b)) for a, b in zip(saved, again))
    torch.autograd.backward([feat, qkv], grads)
    assert all(torch.equal(bits(first[k]), bits(t[k].grad)) for k in t)


def test_no_rows_give_empty_tensors_and_zero_parameter_gradients(dev):
    got = run(fused, make_inputs(0, 32, 96, 1300), dev, torch.float32)
    assert got["feat"].shape == (0, 32) and got["qkv"].shape == (0, 96) and got["dx"].shape == (0, 32)
    assert all(got["d" + k].shape == s and not got["d" + k].any() for k, s in (
        ("wc", (32, 32)), ("bc", (32,)), ("gc", (32,)), ("bec", (32,)), ("g1", (32,)), ("be1", (32,)), ("wq", (96, 32)), ("bq", (96,))))


def test_bad_shapes_are_named(dev):
    from gaussiancity_amd import front
    t = {k: v.to(dev) for k, v in make_inputs(5, 8, 24, 1400).items()}
    args = lambda **kw: [dict(t, **kw)[k] if k in t else v for k, v in (  # noqa: E731
        ("x", 0), ("s", 0), ("wc", 0), ("bc", 0), ("gc", 0), ("bec", 0), ("eps_c", EPS_C), ("g1", 0), ("be1", 0), ("eps_1", EPS_1),
        ("wq", 0), ("bq", 0))]
    with pytest.raises(ValueError, match="lnc_w must be"):
        front.conv_tail_norm_qkv(*args(gc=torch.ones(12, device=dev)))
    with pytest.raises(ValueError, match="s must be"):
        front.conv_tail_norm_qkv(*args(s=torch.ones(4, 8, device=dev)))
    with pytest.raises(ValueError, match="bq must be"):
        front.conv_tail_norm_qkv(*args(bq=torch.ones(20, device=dev)))
    wide = front.max_channels() + 4
    w = {k: v.to(dev) for k, v in make_inputs(5, wide, 24, 1401).items()}
    with pytest.raises(ValueError, match="the fused kernels hold"):
        front.conv_tail_norm_qkv(w["x"], w["s"], w["wc"], w["bc"], w["gc"], w["bec"], EPS_C, w["g1"], w["be1"], EPS_1, w["wq"],
                                 w["bq"])
