"""-m gpu: the stage-seam operator of libgcm_hip.so (gcm_seam_*) through gaussiancity_amd.seam and, for
the bit tests, through the C ABI.

Bar.  y, dx, dw, db, dg, dh and the two running statistics against the float64 formulation on the CPU, at most 4 x the
figure of torch's float32 ops on the same GPU and never below 2^-23 (tests/seam_ref.py; db under batch statistics against
dw's maximum), worst over N in {2, 63, 64, 65, 257}, training and eval mode, with and without the GELU, per (I, O) in
{(4, 4) below a tile, (32, 64), (48, 36) between templates, (128, 132) and (132, 128) across one column block and one input
chunk, (512, 256) and (256, 512) at the cap}, with the product and without it (width O).  One column of z has a mean of
100 standard deviations.  Training and eval use the same inputs, with non-trivial running statistics.
Bits.  Two runs agree, also at N = 64 * 64 + 65 where the grouped fold is on; outputs, z, statistics and workspace
pre-filled with NaN and with 3.0 come back fully written; every proper subset of {dx, dw, db, dg, dh} has the bits of the
full call; two backwards over one retained graph agree and leave the saved tensors unchanged; strided x, y and dy have the
bits of the contiguous call and the padding keeps its fill; the counter goes up by exactly 1 per training forward and by 0
in eval, where the running buffers are untouched; a forward + backward does not wait; with I = 4 and inputs whose chain is
exact the eval-mode z equals F.linear's bits."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import seam_ref as R
from seam_direct import BACKWARD, FORWARD, Direct as _Direct, differing as _same

pytestmark = pytest.mark.gpu
NS = (2, 63, 64, 65, 257)
SHAPES = ((4, 4), (32, 64), (48, 36), (128, 132), (132, 128), (512, 256), (256, 512))
BIG = 64 * 64 + 65


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _cases(I, O, product):
    return [(R.make_inputs(N, I, O, 1000 * I + 10 * O + N, product), training, act)
            for N in NS for training in (True, False) for act in (True, False)]


@pytest.mark.parametrize("I,O", SHAPES)
@pytest.mark.parametrize("product", (True, False))
def test_linear_bn_gelu_meets_the_bar(dev, I, O, product):
    R.check_bar("I = %d, O = %d%s" % (I, O, "" if product else ", no product"), _cases(I, O, product), dev)


@pytest.mark.parametrize("I,O", ((48, 36), (132, 128)))
def test_strided_rows_have_the_bits_of_the_contiguous_call(dev, I, O):
    for product, training in itertools.product((True, False), (True, False)):
        inp = R.make_inputs(65, I, O, 9000 + I, product)
        a = R.run(R.fused, inp, dev, torch.float32, training, True, strided=True)[0]
        b = R.run(R.fused, inp, dev, torch.float32, training, True)[0]
        assert R.same_bits(a, b), (product, training)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,I,O", ((257, 48, 36), (257, 132, 128), (BIG, 32, 64)))
@pytest.mark.parametrize("product", (True, False))
@pytest.mark.parametrize("training", (True, False))
def test_two_runs_agree_and_every_output_is_written_whole_whatever_the_memory_held(dev, N, I, O, product, training):
    """NaN and 3.0 as fills of the outputs, z, the statistics, the workspace and (strided rows) the padding columns: the two
    calls agree bit for bit (so nothing reads what it did not write and nothing is left unwritten), the padding keeps its
    fill, and a third call agrees with the first."""
    p = _Direct(dev, N, I, O, 11 * N + O, product, pad=4)
    nan, three = float("nan"), 3.0
    f1, f2, f3 = p.forward(training, nan), p.forward(training, three), p.forward(training, nan)
    skip = ("y_wide",) + (() if training else ("mean",))
    names = [k for k in FORWARD if k not in skip]
    assert not _same(f1, f2, names) and not _same(f1, f3, names)
    assert not torch.isnan(f1["y"]).any() and torch.isnan(f1["y_wide"][:, O:]).all() and bool((f2["y_wide"][:, O:] == three).all())
    assert int(f1["tracked"]) == 7 + int(training)
    if not training:
        assert torch.equal(f1["running_mean"], p.t["running_mean"]) and torch.equal(f1["running_var"], p.t["running_var"])
    b1, b2, b3 = p.backward(f1, training, nan), p.backward(f1, training, three), p.backward(f1, training, nan)
    names = [k for k in BACKWARD if k != "dx_wide"]
    assert not _same(b1, b2, names) and not _same(b1, b3, names)
    for k in R.GRADS:
        assert b1[k] is None or not torch.isnan(b1[k]).any(), k
    assert torch.isnan(b1["dx_wide"][:, p.I:]).all() and bool((b2["dx_wide"][:, p.I:] == three).all())


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("product", (True, False))
def test_strided_x_y_dy_and_dx_through_the_c_abi_have_the_bits_of_the_contiguous_call(dev, training, product):
    wide, dense = (_Direct(dev, 130, 132, 68, 5, product, pad=pad) for pad in (4, 0))
    fw, fd = wide.forward(training, float("nan")), dense.forward(training, float("nan"))
    assert fw["y"].stride(0) == 72 and fd["y"].stride(0) == 68 and fw["x"].stride(0) == wide.I + 4
    assert not _same(fw, fd, ("y", "z", "mean", "rstd", "running_mean", "running_var", "tracked"))
    bw, bd = wide.backward(fw, training, float("nan")), dense.backward(fd, training, float("nan"))
    assert bw["dx"].stride(0) == wide.I + 4 and not _same(bw, bd, R.GRADS)


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("product", (True, False))
def test_every_proper_subset_of_the_gradients_has_the_bits_of_the_full_call(dev, training, product):
    p = _Direct(dev, 130, 132, 68, 5, product)
    fwd = p.forward(training, 0.0)
    full = p.backward(fwd, training, float("nan"))
    grads = [k for k in R.GRADS if product or k not in ("dw", "db")]
    for r in range(len(grads)):
        for subset in itertools.combinations(grads, r):
            got = p.backward(fwd, training, float("nan"), subset)
            assert not _same(got, {k: full[k] if k in subset else None for k in grads}, grads), subset


@pytest.mark.parametrize("training", (True, False))
def test_two_backwards_over_one_retained_graph_agree_and_leave_the_saved_tensors_unchanged(dev, training):
    inp = R.make_inputs(130, 48, 36, 17)
    first, (y, leaf, dy, _) = R.run(R.fused, inp, dev, torch.float32, training, True, retain=True)
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    before = [t.detach().clone() for t in saved]
    for t in leaf.values():
        t.grad = None
    y.backward(dy)
    for k in R.LEAVES:
        assert torch.equal(R.bits(leaf[k].grad.cpu()), R.bits(first["d" + k])), k
    assert all(torch.equal(R.bits(a), R.bits(b)) for a, b in zip(before, saved))


def test_the_saved_tensors_are_x_z_mean_rstd_and_parameters_never_u_or_y(dev):
    inp = R.make_inputs(70, 32, 64, 3)
    _, (y, leaf, _, _) = R.run(R.fused, inp, dev, torch.float32, True, True, retain=True)
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    before = [t.detach().clone() for t in saved]
    shapes = sorted(tuple(t.shape) for t in saved)
    assert shapes == sorted([(70, 32), (70, 64), (64,), (64,), (64, 32), (64,), (64,)])
    assert not any(t.data_ptr() == y.data_ptr() for t in saved)
    z = F.linear(leaf["x"], leaf["w"], leaf["b"]).detach()
    rows = [t for t in saved if tuple(t.shape) == (70, 64)]
    assert len(rows) == 1 and torch.allclose(rows[0], z, rtol=1e-5, atol=1e-5)        # the one [N, O] tensor kept is z
    y.backward(torch.ones_like(y))
    assert all(torch.equal(R.bits(a), R.bits(b)) for a, b in zip(before, saved))


def test_the_counter_goes_up_by_one_per_training_forward_and_eval_touches_no_buffer(dev):
    from gaussiancity_amd import seam
    inp = {k: None if v is None else v.to(dev) for k, v in R.make_inputs(65, 32, 64, 8).items()}
    args = (inp["x"], inp["w"], inp["b"], inp["g"], inp["h"], inp["running_mean"], inp["running_var"], inp["tracked"])
    kw = dict(momentum=R.MOMENTUM, eps=R.EPS)
    for k in range(3):
        seam.linear_bn_gelu(*args, training=True, **kw)
        assert int(inp["tracked"]) == 7 + k + 1
    mean, var = inp["running_mean"].clone(), inp["running_var"].clone()
    for _ in range(2):
        seam.linear_bn_gelu(*args, training=False, **kw)
    assert int(inp["tracked"]) == 10 and torch.equal(inp["running_mean"], mean) and torch.equal(inp["running_var"], var)


def test_forward_and_backward_do_not_wait(dev):
    from gaussiancity_amd import seam
    seam.max_channels()
    for product, training in itertools.product((True, False), (True, False)):
        inp = R.make_inputs(BIG if training and product else 300, 32, 64, 21, product)
        t = {k: None if inp[k] is None else inp[k].to(dev).requires_grad_(True) for k in R.LEAVES}
        buf = {k: inp[k].to(dev) for k in ("running_mean", "running_var", "tracked")}
        dy = inp["dy"].to(dev)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            y = R.fused(t, buf, training, True)
            y.backward(dy)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert all(t[k].grad is not None for k in R.LEAVES if t[k] is not None)


def test_the_eval_mode_z_has_f_linears_bits_when_the_chain_is_exact(dev):
    """I = 4: the chain is one MFMA step.  x and w are multiples of 1 / 8 of magnitude at most 4 and b a multiple of 1 / 64,
    so every product and partial sum is exact in float32 and float64 alike: z is the float64 value, and any order gives it."""
    N, I, O = 257, 4, 36
    p = _Direct(dev, N, I, O, 4242)
    g = torch.Generator().manual_seed(1)
    eighths = lambda *s: torch.randint(-32, 33, s, generator=g).float() / 8  # noqa: E731
    x, w, b = eighths(N, I), eighths(O, I), torch.randint(-64, 65, (O,), generator=g).float() / 64
    z64 = x.double() @ w.double().T + b.double()
    assert torch.equal(z64.float().double(), z64)
    p.t.update(x=x.to(dev), w=w.to(dev), b=b.to(dev))
    out = p.forward(False, float("nan"))
    assert torch.equal(R.bits(out["z"]), R.bits(F.linear(p.t["x"], p.t["w"], p.t["b"])))
    assert torch.equal(out["z"].cpu().double(), z64)
    u = F.batch_norm(out["z"], p.t["running_mean"], p.t["running_var"], p.t["g"], p.t["h"], False, R.MOMENTUM, R.EPS)
    assert torch.allclose(out["y"], F.gelu(u), rtol=1e-5, atol=1e-6)
