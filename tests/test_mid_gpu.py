"""-m gpu: the Block-middle operators of libgcm_hip.so (gcm_mid_*) through gaussiancity_amd.mid and,
for the bit tests, through the C ABI.

Bar.  y, da, dwp and dbp against the float64 formulation on the CPU, at most 4 x the figure of torch's float32 ops on the
same GPU and never below 2^-23 (tests/mid_ref.py), worst over N in {1, 63, 64, 65, 257} and D in {0 (identity and a
permutation), 1, one value between, N} per C in {4 (below a tile), 32 (a template's width), 48 (between templates), 128 (the
cap)}, with and without a row scale of zeros and 1 / keep.
Bits.  slot_plan equals its numpy formulation; the gather and its gradient equal torch's x[order] and its index_put backward
(W in {12, 96, 384}, contiguous and strided); dx is the incoming gradient; da is +0 at the duplicate slots; the epilogue
equals torch's elementwise ops on the same p (C = 4, inputs whose chain is exact); two runs agree, also beyond 64 row tiles;
outputs and workspace pre-filled with NaN and with 3.0 come back fully written; every proper subset of {da, dwp, dbp} has the
bits of the full call; two backwards over one retained graph agree and leave the saved tensors unchanged."""
import itertools

import pytest
import torch

import mid_ref as R

pytestmark = pytest.mark.gpu
NS = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def index_cases(N):
    """(D, identity): no duplicate with the identity and with a permutation, one, one value between, every row."""
    cases = [(0, True), (0, False), (1, False), (N, False)]
    if N > 2:
        cases.append((N // 3, False))
    return cases


def _cases(C, scale):
    return [R.make_inputs(N, D, C, 1000 * C + 10 * N + k, scale=scale, identity=ident)
            for N in NS for k, (D, ident) in enumerate(index_cases(N))]


@pytest.mark.parametrize("N", NS + (4097,))
def test_slot_plan_equals_the_numpy_formulation(dev, N):
    from gaussiancity_amd import mid
    for D, ident in index_cases(N):
        order, inverse, extra = R.make_indices(N, D, 77 + N + D, ident)
        got = mid.slot_plan(order.to(dev), inverse.to(dev), check=True).cpu()
        assert got.dtype == torch.int32 and torch.equal(got, torch.from_numpy(R.extra_numpy(order, inverse))), (N, D)
        assert torch.equal(got, extra) and int((got >= 0).sum()) == D


def test_slot_plan_check_names_the_broken_rule(dev):
    from gaussiancity_amd import mid
    order, inverse, _ = R.make_indices(65, 7, 5)
    twice = torch.cat([order, order[inverse[3:4]]])                  # row 3 a second time: it may now have two duplicates
    twice = torch.cat([twice, order[inverse[3:4]]])
    with pytest.raises(ValueError, match="at most one duplicate slot per row"):
        mid.slot_plan(twice.to(dev), inverse.to(dev), check=True)
    wrong = inverse.clone()
    wrong[[0, 1]] = inverse[[1, 0]]
    with pytest.raises(ValueError, match=r"order\[inverse\[n\]\] == n"):
        mid.slot_plan(order.to(dev), wrong.to(dev), check=True)
    beyond = order.clone()
    beyond[5] = 65
    with pytest.raises(ValueError, match="rows 0 .. N-1"):
        mid.slot_plan(beyond.to(dev), inverse.to(dev), check=True)
    assert mid.slot_plan(beyond.to(dev), inverse.to(dev)).shape == (65,)   # unchecked: skipped on the device, no wait


@pytest.mark.parametrize("W", (12, 96, 384))
@pytest.mark.parametrize("strided", (False, True))
def test_gather_rows_and_its_gradient_have_torchs_bits(dev, W, strided):
    from gaussiancity_amd import mid
    mid.reset_stats()
    for N in NS:
        for D, ident in index_cases(N):
            inp = R.make_inputs(N, D, 4, 31 * W + N + D, W=W, identity=ident)
            got = R.run(R.fused, inp, dev, torch.float32, strided)[0]
            want = R.run(R.torch_ops, inp, dev, torch.float32)[0]
            assert got["packed"].shape == (N + D, W) and torch.equal(got["packed"], want["packed"]), (N, D)
            assert torch.equal(got["dqkv"], want["dqkv"]), (N, D)
    assert mid.stats()["gather_forward_calls"] == mid.stats()["gather_backward_calls"] > 0


@pytest.mark.parametrize("C", (4, 32, 48, 128))
@pytest.mark.parametrize("scale", (False, True))
def test_proj_residual_meets_the_bar(dev, C, scale):
    R.check_bar("C = %d%s" % (C, ", row scale" if scale else ""), _cases(C, scale), dev)


@pytest.mark.parametrize("C", (48, 128))
def test_strided_rows_go_straight_through(dev, C):
    cases = [R.make_inputs(N, N // 3, C, 9000 + C + N) for N in (65, 257)]
    R.check_bar("C = %d, strided" % C, cases, dev, strided=True)
    for inp in cases:
        assert R.same_bits(R.run(R.fused, inp, dev, torch.float32, True)[0], R.run(R.fused, inp, dev, torch.float32)[0])


def test_the_epilogue_has_torchs_bits_given_the_same_p(dev):
    """C = 4: the chain is one MFMA step.  a and wp are multiples of 1 / 8 of magnitude at most 4 and bp a multiple of
    1 / 64, so every product and partial sum is exact in float32 and float64 alike and p is the float64 value, rounded
    (exactly representable); x and the row scale are arbitrary float32."""
    from gaussiancity_amd import mid
    N, D, C = 257, 40, 4
    inp = R.make_inputs(N, D, C, 4242)
    g = torch.Generator().manual_seed(1)
    eighths = lambda *s: torch.randint(-32, 33, s, generator=g).float() / 8  # noqa: E731
    a, wp, bp = eighths(N + D, C), eighths(C, C), torch.randint(-64, 65, (C,), generator=g).float() / 64
    p64 = a.double()[inp["inverse"]] @ wp.double().T + bp.double()
    p = p64.float()
    assert torch.equal(p.double(), p64)
    x, r = inp["x"].to(dev), inp["r"].to(dev)
    args = (a.to(dev), inp["inverse"].to(dev), inp["extra"].to(dev), x, wp.to(dev), bp.to(dev))
    assert torch.equal(R.bits(mid.proj_residual(*args)), R.bits(x + p.to(dev)))
    assert torch.equal(R.bits(mid.proj_residual(*args, r)), R.bits(x + p.to(dev) * r[:, None]))
    assert torch.equal(R.bits(mid.proj_residual(*args, r[:, None])), R.bits(x + p.to(dev) * r[:, None]))


@pytest.mark.parametrize("N,D,C", ((257, 85, 48), (4097, 1300, 32), (4097, 4097, 128)))
def test_two_runs_agree_in_every_bit(dev, N, D, C):
    inp = R.make_inputs(N, D, C, N + C)
    first, second = (R.run(R.fused, inp, dev, torch.float32)[0] for _ in range(2))
    assert R.same_bits(first, second)
    if N > 4096:   # more than 64 row tiles: the figures once more, at the size where the slices are at their cap
        R.check_bar("N = %d, C = %d" % (N, C), [inp], dev)


# ---- through the C ABI --------------------------------------------------------------------------------------------------------
def _abi_backward(inp, dev, outs=("da", "dwp", "dbp"), fill=float("nan")):
    from gaussiancity_amd import _native_m as M
    lib = M.lib()
    a, wy, wp = (inp[k].to(dev) for k in ("a", "wy", "wp"))
    inverse, extra, r = inp["inverse"].to(dev), inp["extra"].to(dev), inp["r"].to(dev)
    (T, C), N = a.shape, wy.shape[0]
    shapes = {"da": (T, C), "dwp": (C, C), "dbp": (C,)}
    res = {k: torch.full(shapes[k], fill, device=dev) for k in outs}
    need = lib.gcm_mid_backward_workspace_bytes(N, C)
    ws = torch.full((need // 4,), fill, device=dev)
    ptr = lambda k: res[k].data_ptr() if k in res else None  # noqa: E731
    M.check(lib.gcm_mid_backward(a.data_ptr(), C, inverse.data_ptr(), extra.data_ptr(), wy.data_ptr(), C, wp.data_ptr(),
                                 r.data_ptr(), N, T, C, ptr("da"), ptr("dwp"), ptr("dbp"), ws.data_ptr(), need, None),
            "gcm_mid_backward")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


@pytest.mark.parametrize("N,D,C", ((65, 21, 4), (257, 85, 48), (257, 257, 128)))
def test_prefilled_outputs_and_workspace_come_back_fully_written_and_subsets_agree(dev, N, D, C):
    from gaussiancity_amd import _native_m as M
    inp = R.make_inputs(N, D, C, 555 + N + C)
    full = _abi_backward(inp, dev)
    assert all(bool(torch.isfinite(v).all()) for v in full.values())
    other = _abi_backward(inp, dev, fill=3.0)
    assert all(torch.equal(R.bits(full[k]), R.bits(other[k])) for k in full)
    op = R.run(R.fused, inp, dev, torch.float32)[0]                        # the autograd layer calls the same function
    assert all(torch.equal(R.bits(full[k]), R.bits(op[k])) for k in full)
    for size in (1, 2):
        for outs in itertools.combinations(("da", "dwp", "dbp"), size):
            part = _abi_backward(inp, dev, outs)
            assert set(part) == set(outs) and all(torch.equal(R.bits(part[k]), R.bits(full[k])) for k in outs), outs
    # the forward and the two gathers the same way
    lib = M.lib()
    a, x, wp, bp, qkv, wg = (inp[k].to(dev) for k in ("a", "x", "wp", "bp", "qkv", "wg"))
    order, inverse, extra, r = (inp[k].to(dev) for k in ("order", "inverse", "extra", "r"))
    W = qkv.shape[1]
    for fill in (float("nan"), 3.0):
        y, packed, dq = (torch.full(s, fill, device=dev) for s in ((N, C), (N + D, W), (N, W)))
        M.check(lib.gcm_mid_forward(a.data_ptr(), C, inverse.data_ptr(), x.data_ptr(), C, wp.data_ptr(), bp.data_ptr(),
                                    r.data_ptr(), N, C, y.data_ptr(), C, None), "gcm_mid_forward")
        M.check(lib.gcm_mid_gather_forward(qkv.data_ptr(), W, order.data_ptr(), N + D, W, packed.data_ptr(), None), "gather")
        M.check(lib.gcm_mid_gather_backward(wg.data_ptr(), W, inverse.data_ptr(), extra.data_ptr(), N, W, dq.data_ptr(), None),
                "gather backward")
        assert torch.equal(packed, qkv[order]) and torch.equal(dq.cpu(), op["dqkv"])
        assert torch.equal(R.bits(y.cpu()), R.bits(op["y"]))


def test_two_backwards_over_one_retained_graph_agree(dev):
    from gaussiancity_amd import mid
    inp = R.make_inputs(257, 85, 48, 808)
    t = {k: inp[k].to(dev).requires_grad_(True) for k in R.LEAVES}
    wg, wy = inp["wg"].to(dev), inp["wy"].to(dev)
    packed, y = R.fused(t, *(inp[k].to(dev) for k in ("order", "inverse", "extra", "r")))
    held = lambda: [s for f in (packed.grad_fn, y.grad_fn) for s in f.saved_tensors if s is not None]  # noqa: E731
    before, fed = [s.clone() for s in held()], (wg.clone(), wy.clone())
    assert len(before) == 2 + 5                                   # (inverse, extra) and (a, inverse, extra, wp, row_scale)
    mid.reset_stats()
    grads = []
    for _ in range(2):
        for leaf in t.values():
            leaf.grad = None
        torch.autograd.backward([packed, y], [wg, wy], retain_graph=True)
        grads.append({k: leaf.grad.clone() for k, leaf in t.items()})
    assert all(torch.equal(R.bits(grads[0][k]), R.bits(grads[1][k])) for k in R.LEAVES)
    assert all(torch.equal(a, b) for a, b in zip(before, held())) and torch.equal(fed[0], wg) and torch.equal(fed[1], wy)
    assert mid.stats()["backward_calls"] == 2 and mid.stats()["gather_backward_calls"] == 2


def test_only_the_gradients_asked_for_are_computed(dev):
    from gaussiancity_amd import mid
    inp = R.make_inputs(65, 21, 32, 909)
    full = R.run(R.fused, inp, dev, torch.float32)[0]
    for need in (("a",), ("wp", "bp"), ("x",), ("qkv", "bp")):
        mid.reset_stats()
        part = R.run(R.fused, inp, dev, torch.float32, need=need)[0]
        for k in R.LEAVES:
            if k in need:
                assert torch.equal(R.bits(part["d" + k]), R.bits(full["d" + k])), (need, k)
            else:
                assert part["d" + k] is None, (need, k)
        assert mid.stats()["backward_calls"] == (0 if need == ("x",) else 1)   # the shortcut's gradient needs no launch


def test_a_forward_alone_needs_no_plan(dev):
    from gaussiancity_amd import mid
    inp = R.make_inputs(257, 85, 48, 1010)
    t = {k: inp[k].to(dev) for k in R.LEAVES}
    order, inverse, extra, r = (inp[k].to(dev) for k in ("order", "inverse", "extra", "r"))
    with_plan = R.fused(t, order, inverse, extra, r)
    mid.reset_stats()
    for grad_mode in (torch.no_grad, torch.enable_grad):                      # no leaf requires a gradient in either
        with grad_mode():
            without = R.fused(t, order, inverse, None, r)
        assert all(torch.equal(R.bits(a), R.bits(b)) and not b.requires_grad for a, b in zip(with_plan, without))
    assert mid.stats()["plan_calls"] == 0 and mid.stats()["forward_calls"] == 2
    t["a"].requires_grad_(True)
    with pytest.raises(ValueError, match="extra .* is required when a gradient is"):
        mid.proj_residual(t["a"], inverse, None, t["x"], t["wp"], t["bp"])
    with torch.no_grad():
        assert torch.equal(mid.proj_residual(t["a"], inverse, None, t["x"], t["wp"], t["bp"], r), with_plan[1])
    t["qkv"].requires_grad_(True)
    with pytest.raises(ValueError, match="extra .* is required when a gradient is"):
        mid.gather_rows(t["qkv"], order, inverse)
