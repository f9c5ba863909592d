"""-m gpu: the kernels of libgcm_hip.so through gaussiancity_amd.modlinear against float64 numpy.

The bar is tests/test_sparse_gpu.py's: every element within 1e-5 * (the sum of the absolute values of its terms) of the
float64 evaluation -- about a hundred times what a float32 fmaf chain of these lengths loses, and zero where an element
has no term at all (rows without a group, empty groups: those must be exact zeros).  The terms:

    y        sum_i |x_i a_i W_oi| + |beta_o| + |b_o|              dW_oi    sum_r |dpre_ro x_ri a_i|
    dx_i     |a_i| sum_o |dpre_o W_oi|                            dalpha_gi  sum_{r in g} |x_ri| sum_o |dpre_ro W_oi|
    dbeta_go, dbias_o    sum |dpre_ro|

dpre = dy * (y > 0 ? 1 : slope) is the header's rule on the STORED y, so the reference takes the sign from the y the
forward stored (an element whose float64 value is within rounding of 0 has no sign to agree on).

Cases, the reference, the runner and the bar are in tests/modlinear_ref.py, shared with tests/test_modlinear_plans_gpu.py."""
import numpy as np
import pytest
import torch

from modlinear_ref import HEAD_FACTORS, exact_zeros, head_reference, hold, make_case, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


SHAPES = [(N, I, O) for N in (1, 63, 64, 65, 333) for (I, O) in ((4, 4), (20, 36), (64, 64))]


@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("slope,bias", [(0.2, True), (1.0, False)])
@pytest.mark.parametrize("N,I,O", SHAPES)
def test_forward_and_backward_within_the_bar(dev, N, I, O, slope, bias, G):
    c = make_case(N, I, O, G, slope, bias, seed=N * 1000 + I * 10 + G)
    got = run(dev, c)
    hold(c, got, "N%d I%d O%d G%d" % (N, I, O, G))
    exact_zeros(c, got)
    if G == 5 and N >= 63:
        assert (c["group"] < 0).any() and not (c["group"] == 3).any() and len(np.unique(c["group"])) == 5


@pytest.mark.parametrize("slope,bias", [(0.2, False), (1.0, True)])
def test_the_other_two_combinations_of_slope_and_bias(dev, slope, bias):
    c = make_case(65, 20, 36, 5, slope, bias, seed=11)
    got = run(dev, c)
    hold(c, got, "slope %g bias %s" % (slope, bias))
    exact_zeros(c, got)


def test_the_real_reduction_length(dev):
    """512 x 512 at N = 130: 32 staged slices per product, two row slices of dW, rows of five groups in every tile."""
    c = make_case(130, 512, 512, 5, 0.2, True, seed=512)
    got = run(dev, c)
    hold(c, got, "512x512")
    exact_zeros(c, got)


@pytest.mark.parametrize("N", [65, 333])
def test_plain_linear_layer_without_alpha_beta_and_group(dev, N):
    c = make_case(N, 20, 36, 1, 0.2, True, seed=N, plain=True)
    got = run(dev, c)
    assert sorted(got) == ["dbias", "dw", "dx", "y"]
    hold(c, got, "plain N%d" % N)


def test_row_strided_input_gives_the_contiguous_result_bit_for_bit(dev):
    c = make_case(65, 20, 36, 5, 0.2, True, seed=7)
    got, dense = run(dev, c, strided=True), run(dev, c)
    hold(c, got, "strided")
    assert all(got[k].tobytes() == dense[k].tobytes() for k in dense)


def test_two_backward_runs_are_bit_identical(dev):
    for shape in ((333, 64, 64, 5), (130, 512, 512, 5), (333, 20, 36, 1)):
        c = make_case(*shape, 0.2, True, seed=3)
        first, second = run(dev, c), run(dev, c)
        assert sorted(first) == ["dalpha", "dbeta", "dbias", "dw", "dx", "y"]
        assert all(first[k].tobytes() == second[k].tobytes() for k in first), shape


def test_no_rows(dev):
    """N = 0: both calls return, y and dx are empty, dW and the per-group gradients are zeros."""
    c = make_case(0, 20, 36, 5, 0.2, True, seed=1)
    got = run(dev, c)
    assert got["y"].shape == (0, 36) and got["dx"].shape == (0, 20)
    for name, shape in (("dw", (36, 20)), ("dalpha", (5, 20)), ("dbeta", (5, 36)), ("dbias", (36,))):
        assert got[name].shape == shape and not got[name].any(), name


@pytest.mark.parametrize("G", [1, 3, 300])
def test_groups_from_masks_is_the_python_loop(dev, G):
    from gaussiancity_amd.modlinear import groups_from_masks
    n = 1000
    rng = np.random.default_rng(G)
    masks = rng.random((G, n)) < (0.6 if G <= 3 else 0.01)   # overlapping: a row may be set in several masks
    if G > 1:
        masks[G // 2] = False                                # an all-false mask
        assert (masks.sum(0) > 1).any()
    else:
        assert not masks.all()
    want = np.full(n, -1, np.int32)
    for g in range(G):
        want[masks[g]] = g                                   # upstream's loop: a later assignment wins
    got = groups_from_masks([torch.from_numpy(m).to(dev) for m in masks], n)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert (want == -1).any() and (G == 1 or not (want == G // 2).any())
    shaped = groups_from_masks([torch.from_numpy(m).to(dev).reshape(1, n) for m in masks], n)   # upstream's [1, n] masks
    assert np.array_equal(shaped.cpu().numpy(), want)


def test_groups_from_masks_all_false(dev):
    from gaussiancity_amd.modlinear import groups_from_masks
    got = groups_from_masks([torch.zeros(1000, dtype=torch.bool, device=dev)], 1000)
    assert (got == -1).all()


@pytest.mark.parametrize("kind", ["xyz", "rgb", "scale", "opacity"])
def test_head_out_against_float64(dev, kind):
    """Within 1e-5 * (sum_i |f_i W_ci| + |b_c|) * |transform'| plus one float32 unit of the result.  The clamp of `scale`
    has slope `factor` inside and 0 outside; a value within the bar of the clamp's corner may sit on either side of it,
    so the slope there is `factor` (the transform's Lipschitz constant)."""
    from gaussiancity_amd.modlinear import head_out
    N, I, C, factor = 333, 52, 1 if kind == "opacity" else 3, HEAD_FACTORS[kind]
    rng = np.random.default_rng(len(kind))
    f = rng.normal(size=(N, I)).astype(np.float32)
    w = (rng.normal(size=(C, I)) * 1.5 / np.sqrt(I)).astype(np.float32)
    b = (rng.normal(size=C) * 0.2).astype(np.float32)
    group = rng.integers(-1, 4, size=N).astype(np.int32)
    v, want, bar = head_reference(kind, f, w, b, factor)
    if kind == "scale":
        inside = np.abs(v[group >= 0]) < 1
        assert inside.any() and (~inside).any(), "the clamp must be active on some rows and inactive on others"
    for grp in (group, None):
        live = (grp >= 0)[:, None] if grp is not None else np.ones((N, 1), bool)
        got = head_out(torch.from_numpy(f).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev),
                       None if grp is None else torch.from_numpy(grp).to(dev), kind, factor)
        assert got.dtype == torch.float32 and tuple(got.shape) == (N, C)
        got = got.cpu().numpy()
        assert not got[~live[:, 0]].any()                    # rows without a group: exact zeros
        err = np.abs(got.astype(np.float64) - want) * live
        print("%s worst error / bar %.3f" % (kind, float((err / bar).max())))
        assert (err <= bar).all(), (kind, float((err / bar).max()))
