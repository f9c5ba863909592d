"""-m gpu: the stage-seam operator (gcm_seam_*) beyond the five row tiles of tests/test_seam_gpu.py: the
two-level folds of k_seam_stats and k_seam_bwd_fold and the capped slice plans of k_seam_dw, at the shapes of
tests/seam_plans.py's PLAN_CASES (tests/test_seam_host.py ties each shape to the branch it names without a GPU).

Values are held to test_seam_gpu.py's bar (tests/seam_ref.py): float64 on the CPU is the target, the torch float32
formulation on the same GPU the yardstick, per tensor at most max(4 x yardstick, 2^-23), per shape from its own yardstick
only; every figure is printed before anything is asserted.  Every input here drifts: a ramp of 50 over the rows on one
column of x (make_inputs' drift), so that the tiles' means differ by many standard deviations, as rows ordered along a
space-filling curve do, and the between-tile part count_t (mean_t - mean)^2 carries most of the variance.

  plan cases   training and eval, with and without the GELU, one bar per shape; with the product for all seven shapes,
               without it (width O: k_seam_tile_stats, k_seam_apply, k_seam_dz) for NO_PRODUCT_CASES.
  full weight  the training cases of STATISTICS_CASES again with momentum = 1.0: running_mean and running_var are then the
               batch mean and the unbiased batch variance and meet the same bar undamped.
  saved        mean and rstd as gcm_seam_forward_train stores them against z.double().mean(0) and (var + eps)^-1/2 of the z
               the kernel stored, max|got - x64| / max|x64| at most max(4 x torch float32's figure, 2^-23).
  subsets      at (4097, 132, 128) -- group records, the `keep` piece and slice records all live -- every proper subset of
               {dx, dw, db, dg, dh} has the bits of the full call.
  fills        at (262209, 4, 4), G at its cap: outputs and workspace pre-filled with NaN and with 3.0 come back identical
               and finite, so no group reads a record that was not written.

Measured on one MI355X, worst ratio operator / yardstick per tensor over everything this file prints (bar 4):
y 1.02, dx 0.99, dw 1.44, db 1.42, dg 2.23, dh 1.18, running_mean 1.74, running_var 2.42 (at momentum 1; 1.01 at 0.01), saved
mean 1.00, saved rstd 0.94.  With a running (count, mean, M2) merge in k_seam_stats and plain sums over the tiles in
k_seam_bwd_fold, as gcm_seam.h once had them: dh 5.35 at (262209, 4, 4), running_var 40.5 there and 27.8 at (16384, 32, 64)
without the product at momentum 1, saved rstd 9.9 / 5.9 / 10.7 at the three STATISTICS_CASES.  Each of three mutations of
the grouped folds (the groups' variance term dropped, a group's last tile dropped in k_seam_bwd_fold, the last group
dropped in both folds) passes all of tests/test_seam_gpu.py and fails 16 to 22 tests here by factors of 10^3 to 10^8 over
the bar."""
import itertools

import pytest
import torch

import seam_plans as P
import seam_ref as R
from seam_direct import BACKWARD, FORWARD, Direct, differing

pytestmark = pytest.mark.gpu
DRIFT = 50.0
SUBSET_SHAPE = (4097, 132, 128)
FILL_SHAPE = (262209, 4, 4)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _seed(N, I, O):
    return 1000 * I + 10 * O + N


def _shapes():
    """(N, I, O, product): every plan case with the product, NO_PRODUCT_CASES also without."""
    return [s + (True,) for s in P.PLAN_CASES] + [s + (False,) for s in P.NO_PRODUCT_CASES]


def _label(N, I, O, product, more=""):
    return "N = %d, I = %d, O = %d%s%s" % (N, I, O, "" if product else ", no product", more)


@pytest.mark.parametrize("N,I,O,product", _shapes())
def test_every_plan_case_meets_the_bar_from_its_own_yardstick(dev, N, I, O, product):
    inp = R.make_inputs(N, I, O, _seed(N, I, O), product, drift=DRIFT)
    cases = [(inp, training, act) for training in (True, False) for act in (True, False)]
    R.check_bar(_label(N, I, O, product), cases, dev)


@pytest.mark.parametrize("product", (True, False))
@pytest.mark.parametrize("N,I,O", P.STATISTICS_CASES)
def test_with_momentum_one_the_running_buffers_are_the_batch_statistics_and_meet_the_bar(dev, N, I, O, product):
    inp = R.make_inputs(N, I, O, _seed(N, I, O), product, drift=DRIFT)
    R.check_bar(_label(N, I, O, product, ", momentum 1"), [(inp, True, act) for act in (True, False)], dev, momentum=1.0)


@pytest.mark.parametrize("product", (True, False))
@pytest.mark.parametrize("N,I,O", P.STATISTICS_CASES)
def test_the_saved_mean_and_rstd_are_those_of_the_stored_z(dev, N, I, O, product):
    """The float64 targets are taken from the z the kernel stored (x itself without a product), so the product's own error is
    not counted again; the yardstick is torch's float32 mean and biased variance of that same z on the GPU."""
    p = Direct(dev, N, I, O, _seed(N, I, O), product)
    p.t["x"] = R.make_inputs(N, I, O, _seed(N, I, O), product, drift=DRIFT)["x"].to(dev)
    out = p.forward(True, float("nan"))
    z = out["z"] if product else out["x"]
    z64 = z.double().cpu()
    want = {"mean": z64.mean(0), "rstd": (z64.var(0, unbiased=False) + R.EPS) ** -0.5}
    yard = {"mean": z.mean(0), "rstd": (torch.var(z, 0, unbiased=False) + R.EPS) ** -0.5}
    failed = []
    for k in ("mean", "rstd"):
        top = float(want[k].abs().max())
        got, ref = (float((t.double().cpu() - want[k]).abs().max()) / top for t in (out[k], yard[k]))
        bar = max(R.FACTOR * ref, R.FLOOR)
        print("%s saved %-4s operator %.3e  torch float32 %.3e  ratio %.2f  bar %.3e" % (
            _label(N, I, O, product), k, got, ref, got / max(ref, 1e-30), bar))
        if not got <= bar:
            failed.append((k, got, bar))
    assert not failed, failed


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("product", (True, False))
def test_every_proper_subset_of_the_gradients_has_the_bits_of_the_full_call_at_a_grouped_size(dev, training, product):
    f = P.facts(SUBSET_SHAPE)
    assert f["G"] >= 2 and f["sw"] >= 2 and f["output_chunks"] == 1 and f["input_chunks"] == 2, f
    p = Direct(dev, *SUBSET_SHAPE, 5, product)
    fwd = p.forward(training, 0.0)
    full = p.backward(fwd, training, float("nan"))
    grads = [k for k in R.GRADS if product or k not in ("dw", "db")]
    assert all(bool(torch.isfinite(full[k]).all()) for k in grads)
    for r in range(len(grads)):
        for subset in itertools.combinations(grads, r):
            got = p.backward(fwd, training, float("nan"), subset)
            assert not differing(got, {k: full[k] if k in subset else None for k in grads}, grads), subset


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("product", (True, False))
def test_at_the_group_cap_two_fills_come_back_identical_and_finite(dev, training, product):
    """tests/test_seam_gpu.py's method at G = kSeamGroups: NaN and 3.0 as fills of the outputs, z, the statistics and the
    workspace; the calls agree bit for bit and nothing that comes back is a NaN or an infinity."""
    f = P.facts(FILL_SHAPE)
    assert f["G_at_cap"] and f["last_group_short"], f
    N, I, O = FILL_SHAPE
    p = Direct(dev, N, I, O, 11 * N + O, product, pad=4)
    nan, three = float("nan"), 3.0
    f1, f2 = p.forward(training, nan), p.forward(training, three)
    names = [k for k in FORWARD if k != "y_wide" and (training or k != "mean")]
    assert not differing(f1, f2, names)
    for k in names:
        assert f1[k] is None or f1[k].dtype != torch.float32 or bool(torch.isfinite(f1[k]).all()), k
    assert torch.isnan(f1["y_wide"][:, O:]).all() and bool((f2["y_wide"][:, O:] == three).all())
    assert int(f1["tracked"]) == 7 + int(training)
    b1, b2 = p.backward(f1, training, nan), p.backward(f1, training, three)
    names = [k for k in BACKWARD if k != "dx_wide"]
    assert not differing(b1, b2, names)
    for k in R.GRADS:
        assert b1[k] is None or bool(torch.isfinite(b1[k]).all()), k
    assert torch.isnan(b1["dx_wide"][:, p.I:]).all() and bool((b2["dx_wide"][:, p.I:] == three).all())
