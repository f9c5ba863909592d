"""-m gpu: every launch plan, gradient subset and stride of the grouped modulated linear layer and of head_out
(gcm_modlinear_*, gcm_head_out) that tests/test_modlinear_gpu.py's shapes (G in {1, 5}, N <= 333,
all five gradients, only x strided) do not reach.

Values are held to test_modlinear_gpu.py's bar (tests/modlinear_ref.py): every element within 1e-5 x the sum of its
absolute terms of float64, exact zeros where there is no term.  The longest single chain of any plan here is 320 rows;
its worst-case rounding, 320 x 2^-24 = 1.9e-5 of that sum, is above the bar only for adversarial signs, and the seeded
normal inputs lose about sqrt(320) x 2^-24 = 1e-6.

  many groups   the counting sort behind dalpha / dbeta / dbias: more groups than k_sort_count has threads, more counts
                than k_sort_scan has threads (a thread owns a run, group starts land inside it).  A row placed in the
                wrong group moves one term of a sum of a few: far outside 1e-5.
  capped plans  the dW slices and the group slices at their caps, slices that have no row.
  out of range  group values outside 0 .. G-1 are rows without a group.
  subsets       each requested gradient has the BITS of the all-five run: every sum has a fixed order and a NULL output
                only removes stores.
  strides       a row-strided weight and a row-strided dy give the bits of the contiguous run.
  head_out      several steps of the 64-wide loop over I, the 16-rows-per-block edge, no bias, a strided f."""
import itertools

import numpy as np
import pytest
import torch

import gcm_plans
from modlinear_ref import GRADS, HEAD_FACTORS, LEAVES, exact_zeros, head_reference, hold, make_case, run, same_bytes

pytestmark = pytest.mark.gpu
MANY_GROUPS = ((1025, 20, 36, 300), (300, 4, 4, 1100), (2049, 4, 4, 5))
CAPPED = ((20000, 4, 4, 1), (2049, 512, 512, 5))
assert sorted(MANY_GROUPS + CAPPED) == sorted(gcm_plans.cases("modlinear"))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("N,I,O,G", MANY_GROUPS)
def test_many_groups_go_through_the_counting_sort_within_the_bar(dev, N, I, O, G):
    c = make_case(N, I, O, G, 0.2, True, seed=N + G)
    sizes = np.bincount(c["group"][c["group"] >= 0], minlength=G)
    assert (c["group"] < 0).any() and (sizes == 0).any() and (sizes > 1).any() and (G == 5 or (sizes == 1).sum() >= 10)
    assert N % 128 != 1 or c["group"][N - 1] >= 0      # at N = 128 k + 1 the last row is all the last dW slice has
    got = run(dev, c)
    hold(c, got, "N%d I%d O%d G%d" % (N, I, O, G))
    exact_zeros(c, got)


@pytest.mark.parametrize("N,I,O,G", CAPPED)
def test_slice_counts_at_their_caps_and_slices_without_rows_within_the_bar(dev, N, I, O, G):
    facts = gcm_plans.facts("modlinear", (N, I, O, G))
    assert facts["sw_at_cap"] and facts["empty_slices"] >= 1, facts
    c = make_case(N, I, O, G, 0.2, True, seed=N + I)
    got = run(dev, c)
    hold(c, got, "N%d I%d O%d G%d" % (N, I, O, G))
    exact_zeros(c, got)


@pytest.mark.parametrize("N,I,O,G", [(333, 20, 36, 5), (1025, 20, 36, 300)])
def test_group_values_outside_the_range_are_rows_without_a_group(dev, N, I, O, G):
    c = make_case(N, I, O, G, 0.2, True, seed=41)
    bare = np.flatnonzero(c["group"] < 0)
    assert len(bare) >= 3
    odd = dict(c, group=c["group"].copy())
    odd["group"][bare] = np.resize(np.array([G, G + 7, -2 ** 31], np.int32), len(bare))
    assert {G, G + 7, -2 ** 31} <= set(odd["group"].tolist()) and not (odd["group"] == -1).any()
    got, plain = run(dev, odd), run(dev, c)
    assert not got["y"][bare].any() and not got["dx"][bare].any()
    exact_zeros(odd, got)
    assert sorted(got) == sorted(plain) and same_bytes(got, plain)
    hold(odd, got, "out of range N%d G%d" % (N, G))


def subsets(leaves):
    return [s for k in range(1, len(leaves) + 1) for s in itertools.combinations(leaves, k)]


def hold_subsets(dev, c, leaves):
    full = run(dev, c, need=leaves)
    assert sorted(full) == sorted(["y"] + [GRADS[k] for k in leaves])
    wrong = []
    for need in subsets(leaves):
        got = run(dev, c, need=need)       # (run asserts that a leaf outside `need` has no .grad)
        if sorted(got) != sorted(["y"] + [GRADS[k] for k in need]):
            wrong.append((need, sorted(got)))
        wrong += [(need, k) for k in got if got[k].tobytes() != full[k].tobytes()]
    assert not wrong, wrong[:20]


@pytest.mark.parametrize("N,I,O,G", [(333, 20, 36, 5), (1025, 20, 36, 300)])
def test_every_gradient_subset_gives_the_bits_of_the_all_five_run(dev, N, I, O, G):
    hold_subsets(dev, make_case(N, I, O, G, 0.2, True, seed=51), LEAVES)


def test_every_gradient_subset_of_the_plain_layer_gives_the_bits_of_the_all_three_run(dev):
    hold_subsets(dev, make_case(333, 20, 36, 1, 0.2, True, seed=52, plain=True), ("x", "w", "bias"))


@pytest.mark.parametrize("N,I,O,G", [(20000, 4, 4, 1), (1025, 20, 36, 300)])
def test_nan_prefilled_outputs_and_workspace_come_back_fully_written(dev, N, I, O, G):
    """At the ABI, with a slice of dW that has no row and with a scan run of two: every partial record, count and group
    start is written before it is read, and the results have the bits of the run through autograd."""
    from gaussiancity_amd import _native_m as M
    lib = M.lib()
    c = make_case(N, I, O, G, 0.2, True, seed=71)
    want = run(dev, c)
    d = {k: torch.from_numpy(c[k]).to(dev) for k in ("x", "w", "dy", "alpha", "beta", "bias", "group")}
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)  # noqa: E731
    p = lambda k: d[k].data_ptr()  # noqa: E731
    y = nan(N, O)
    M.check(lib.gcm_modlinear_forward(p("x"), I, p("w"), I, p("alpha"), p("beta"), p("bias"), p("group"), N, I, O, G,
                                      c["slope"], y.data_ptr(), O, None), "forward")
    out = {"dx": nan(N, I), "dw": nan(O, I), "dalpha": nan(G, I), "dbeta": nan(G, O), "dbias": nan(O)}
    need = lib.gcm_modlinear_backward_workspace_bytes(N, I, O, G)
    ws = nan(need // 4 + 1)
    M.check(lib.gcm_modlinear_backward(p("x"), I, y.data_ptr(), O, p("dy"), O, p("w"), I, p("alpha"), p("group"), N, I, O, G,
                                       c["slope"], out["dx"].data_ptr(), I, out["dw"].data_ptr(), out["dalpha"].data_ptr(),
                                       out["dbeta"].data_ptr(), out["dbias"].data_ptr(), ws.data_ptr(), need, None), "backward")
    torch.cuda.synchronize()
    out["y"] = y
    got = {k: v.cpu().numpy() for k, v in out.items()}
    differ = [k for k in want if got[k].tobytes() != want[k].tobytes()]
    assert sorted(got) == sorted(want) and not differ, differ


@pytest.mark.parametrize("N,I,O,G", [(333, 20, 36, 5), (130, 512, 512, 5)])
def test_a_row_strided_weight_and_a_row_strided_dy_give_the_bits_of_the_contiguous_run(dev, N, I, O, G):
    c = make_case(N, I, O, G, 0.2, True, seed=61)
    dense = run(dev, c)
    hold(c, dense, "dense N%d I%d" % (N, I))
    for how in ({"strided_w": True}, {"strided_dy": True}, {"strided": True, "strided_w": True, "strided_dy": True}):
        got = run(dev, c, **how)
        assert sorted(got) == sorted(dense) and same_bytes(got, dense), how


@pytest.mark.parametrize("I", [4, 64, 68, 132, 512])
@pytest.mark.parametrize("kind", ["xyz", "rgb", "scale", "opacity"])
def test_head_out_over_the_width_loop_and_the_block_edge(dev, kind, I):
    """test_modlinear_gpu.py's bar expression (modlinear_ref.head_reference), at widths of one, exactly one, just over
    one, over two and eight steps of the 64-wide loop and at N around the 16 rows of a block; with and without group and
    bias; f contiguous and row-strided, the strided run bit-equal to the contiguous one."""
    from gaussiancity_amd.modlinear import head_out
    C, factor = 1 if kind == "opacity" else 3, HEAD_FACTORS[kind]
    rng = np.random.default_rng(1000 * len(kind) + I)
    w = (rng.normal(size=(C, I)) * 1.5 / np.sqrt(I)).astype(np.float32)
    bias = (rng.normal(size=C) * 0.2).astype(np.float32)
    worst = 0.0
    for N in (1, 15, 16, 17, 333):
        f = rng.normal(size=(N, I)).astype(np.float32)
        group = rng.integers(-1, 4, size=N).astype(np.int32)
        group[0], group[N - 1] = 2, 1                        # the first row and the last row of the last block count
        if N >= 15:
            group[N // 2] = -1
        fd = torch.from_numpy(f).to(dev)
        wide = torch.full((N, I + 8), 7.0, device=dev)
        wide[:, :I] = fd
        for b in (bias, None):
            v, want, bar = head_reference(kind, f, w, b, factor)
            if kind == "scale" and N == 333:
                inside = np.abs(v) < 1
                assert inside.any() and (~inside).any(), "the clamp must be active on some rows and inactive on others"
            for grp in (group, None):
                live = (grp >= 0)[:, None] if grp is not None else np.ones((N, 1), bool)
                args = (torch.from_numpy(w).to(dev), None if b is None else torch.from_numpy(b).to(dev),
                        None if grp is None else torch.from_numpy(grp).to(dev), kind, factor)
                got, strided = head_out(fd, *args), head_out(wide[:, :I], *args)
                assert got.dtype == torch.float32 and tuple(got.shape) == (N, C)
                got = got.cpu().numpy()
                assert got.tobytes() == strided.cpu().numpy().tobytes(), (N, "strided f")
                assert not got[~live[:, 0]].any()            # rows without a group: exact zeros
                err = np.abs(got.astype(np.float64) - want) * live
                worst = max(worst, float((err / bar).max()))
                assert (err <= bar).all(), (kind, I, N, b is None, grp is None, float((err / bar).max()))
    print("%s I=%d worst error / bar %.3f" % (kind, I, worst))
