"""-m gpu: every launch plan, channel width and gradient subset of the feed-forward operator (gcm_ffn_*, DESIGN.md
section 18) that tests/test_ffn_gpu.py's shapes (N <= 257, all seven gradients) do not reach.

Values are held to test_ffn_gpu.py's bar (tests/ffn_ref.py): float64 on the CPU is the target, the torch float32
formulation on the same GPU the yardstick, per tensor at most max(4 x yardstick, 2^-23); both figures are printed.

  large N     the shapes of tests/gcm_plans.py's PLAN_CASES: the two-level LayerNorm fold (k_ffn_fold_groups) with a shorter
              last group, the weight-gradient slices at their cap with slices that have no row.  Dropping one of 65 tile
              records changes dln_w by about 1/65 of its value; the bar is near 1e-6.
  widths      C in 65..127 (NJ = 4 with dead channels), C just over a template boundary, Hd below one staged slice.
  subsets     the backward skips launches and passes NULL outputs by needs_input_grad.  Every sum has a fixed order and
              a NULL output only removes stores, so each requested gradient has the BITS of the all-seven run.
  NaN fill    outputs and workspace pre-filled with NaN at a two-level shape: every record is written before it is read."""
import itertools

import pytest
import torch

import gcm_plans
from ffn_ref import EPS, LEAVES, TENSORS, bits, check_bar, fused, make_inputs, run, same_bits

pytestmark = pytest.mark.gpu
WIDTHS = ((36, 144), (68, 64), (100, 400), (128, 8), (4, 512), (64, 256))
SUBSET_SHAPES = ((130, 48, 40), (4097, 4, 4))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def half_scaled(N, seed):
    """A row scale for every other call: dropped rows (the first among them), kept rows at 1 / 0.7.  The last row is
    kept: at N = 64 k + 1 it is the only row of the last tile, and a dropped row's LayerNorm partials are zeros -- the
    last tile's record, the one a fold that stops early loses, would then hold nothing to lose."""
    s = torch.tensor([0.0, 1.0, 1.0 / 0.7])[torch.randint(0, 3, (N,), generator=torch.Generator().manual_seed(seed))]
    s[0], s[N - 1] = 0.0, 1.0 / 0.7
    return s


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "row_scale"])
@pytest.mark.parametrize("N,C,Hd", gcm_plans.cases("ffn"))
def test_the_two_level_fold_and_the_capped_slices_meet_the_bar(dev, N, C, Hd, scaled):
    facts = gcm_plans.facts("ffn", (N, C, Hd))
    assert facts["groups"] >= 2 and facts["sw_at_cap"] and facts["empty_slices"] >= 1, facts
    inp = make_inputs(N, C, Hd, 1000 + N + C)
    check_bar("N=%d C=%d Hd=%d%s" % (N, C, Hd, " row_scale" if scaled else ""), [(inp, half_scaled(N, N) if scaled else None)], dev)


@pytest.mark.parametrize("C,Hd", WIDTHS)
def test_widths_between_and_just_over_the_template_boundaries_meet_the_bar(dev, C, Hd):
    check_bar("C=%d Hd=%d" % (C, Hd), [(make_inputs(N, C, Hd, 1100 + N), half_scaled(N, N) if N == 130 else None)
                                       for N in (1, 65, 130)], dev)


def subsets_of(N):
    """All 127 subsets on the small shape; on the large one each single leaf and each complement (x alone and
    everything but x among them)."""
    if N <= 256:
        return [c for k in range(1, len(LEAVES) + 1) for c in itertools.combinations(LEAVES, k)]
    return [(k,) for k in LEAVES] + [tuple(j for j in LEAVES if j != k) for k in LEAVES]


@pytest.mark.parametrize("N,C,Hd", SUBSET_SHAPES)
def test_every_gradient_subset_gives_the_bits_of_the_all_seven_run(dev, N, C, Hd):
    inp, s = make_inputs(N, C, Hd, 1200 + N), half_scaled(N, 12)
    full = run(fused, inp, dev, torch.float32, s)
    assert all(full[k] is not None for k in TENSORS)
    wrong = []
    for need in subsets_of(N):
        got = run(fused, inp, dev, torch.float32, s, need=need)
        for leaf in LEAVES:
            k = "d" + leaf
            if leaf not in need:
                if got[k] is not None:
                    wrong.append((need, k, "a gradient nobody asked for"))
            elif got[k] is None:
                wrong.append((need, k, "missing"))
            elif not torch.equal(bits(got[k]), bits(full[k])):
                wrong.append((need, k, "%d elements differ" % int((bits(got[k]) != bits(full[k])).sum())))
        if not torch.equal(bits(got["y"]), bits(full["y"])):
            wrong.append((need, "y", "differs"))
    assert not wrong, wrong[:20]


@pytest.mark.parametrize("only", [None, "dln_w"], ids=["all", "dln_w_alone"])
def test_nan_prefilled_outputs_and_workspace_come_back_fully_written_at_a_two_level_shape(dev, only):
    """test_ffn_gpu.py's ABI-level test at (4097, 4, 4), and once more with dln_w the only output: the group records
    (lngroup) and the records of the slices without rows are written before they are read."""
    from gaussiancity_amd import _native_m as M
    lib, (N, C, Hd) = M.lib(), (4097, 4, 4)
    assert gcm_plans.facts("ffn", (N, C, Hd))["groups"] == 2
    inp = make_inputs(N, C, Hd, 1300)
    want = run(fused, inp, dev, torch.float32)
    d = {k: v.to(dev) for k, v in inp.items()}
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)  # noqa: E731
    y, mean, rstd, a = nan(N, C), nan(N), nan(N), nan(N, Hd)
    p = lambda k: d[k].data_ptr()  # noqa: E731
    M.check(lib.gcm_ffn_forward(p("x"), C, p("ln_w"), p("ln_b"), EPS, p("w1"), p("b1"), p("w2"), p("b2"), None, N, C, Hd,
                                y.data_ptr(), C, mean.data_ptr(), rstd.data_ptr(), a.data_ptr(), None), "forward")
    out = {"dx": nan(N, C), "dln_w": nan(C), "dln_b": nan(C), "dw1": nan(Hd, C), "db1": nan(Hd), "dw2": nan(C, Hd), "db2": nan(C)}
    q = lambda k: out[k].data_ptr() if only in (None, k) else None  # noqa: E731
    need = lib.gcm_ffn_backward_workspace_bytes(N, C, Hd)
    ws = nan(need // 4 + 1)
    M.check(lib.gcm_ffn_backward(p("x"), C, mean.data_ptr(), rstd.data_ptr(), a.data_ptr(), p("dy"), C, None, p("ln_w"),
                                 p("ln_b"), p("w1"), p("w2"), N, C, Hd, q("dx"), C, q("dln_w"), q("dln_b"), q("dw1"), q("db1"),
                                 q("dw2"), q("db2"), ws.data_ptr(), need, None), "backward")
    torch.cuda.synchronize()
    out["y"] = y
    for k in ("mean", "rstd", "a"):
        assert bool(torch.isfinite({"mean": mean, "rstd": rstd, "a": a}[k]).all()), k
    got = {k: v.cpu() for k, v in out.items()}
    if only is None:
        assert same_bits(got, want)
    else:
        assert torch.equal(bits(got["y"]), bits(want["y"])) and torch.equal(bits(got[only]), bits(want[only]))
        untouched = [k for k in out if k not in ("y", only)]
        assert all(bool(torch.isnan(got[k]).all()) for k in untouched), "an output that was passed as NULL was written"
