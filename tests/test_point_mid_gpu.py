"""-m gpu: point_mid's middle of the rebound Block.forward.

Golden.  Against the reference's own SerializedAttention.forward (enable_flash=False, patch 48) followed by the residual
add (tests/golden/ptv3_block_mid.npz, written by tests/golden/make_ptv3_block_mid_golden.py in float64, with the error of
the reference's own float32 run per tensor): two batch elements of 90 and 60 points, 6 and 36 duplicate slots.  The test
runs attn.qkv by torch and point_mid.middle on the GPU; every output and gradient is within 4 x err32 of the fixture.

Composed.  With the real point_front, point_attention and point_ffn on tests/test_point_front_gpu.py's point set and
stand-ins (imported: the Block, the attention and the DropPath written by upstream's behaviour), in both install orders,
against float64 on the CPU as target and float32 on the GPU with nothing installed as yardstick, at that file's bar; after
point_mid.uninstall the outputs have the bits of a run that never installed it.  In training mode with DropPath(0.3) the
middle draws upstream's first mask from the same seed at the same position.  A Block with an active proj_drop, a Block
wider than the cap, an active autocast and CPU tensors go to the lines they went to before, and the counters show it.
Nothing here reads the reference: the fixture and the stand-ins only."""
import os
import types

import numpy as np
import pytest
import torch

import test_point_front_gpu as PF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Block, PT_V3 = PF.Block, PF.PT_V3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_a, _native_m
    _native_m.lib()
    _native_a.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ptv3_block_mid.npz"))


def _modules():
    from gaussiancity_amd import mid, point_attention, point_ffn, point_front, point_mid
    return types.SimpleNamespace(mid=mid, attention=point_attention, ffn=point_ffn, front=point_front, middle=point_mid)


def _reset(m):
    for mod in (m.mid, m.attention, m.ffn, m.front, m.middle):
        mod.reset_stats()


@pytest.fixture()
def clean():
    """Nothing installed before and after; a test installs what it needs."""
    m = _modules()
    own = Block.forward
    _reset(m)
    yield m
    m.middle.uninstall(PT_V3)
    m.front.uninstall(PT_V3)
    m.ffn.uninstall(PT_V3)
    assert Block.forward is own and not [n for n in vars(PT_V3) if n.startswith("_gaussiancity_amd")]


# ---- the golden run ---------------------------------------------------------------------------------------------------------
GOLDEN_PARAMS = {"qkv.weight": lambda b: b.attn.qkv.weight, "qkv.bias": lambda b: b.attn.qkv.bias,
                 "proj.weight": lambda b: b.attn.proj.weight, "proj.bias": lambda b: b.attn.proj.bias}


@pytest.mark.parametrize("case", ["c32", "c64"])
def test_the_middle_matches_the_reference_run(dev, clean, golden, case):
    m = clean
    C = golden[case + ".feat"].shape[1]
    block = Block(C, PF.SerializedAttention(C, C // 16, 48), tail=False).to(dev)
    with torch.no_grad():
        for name, get in GOLDEN_PARAMS.items():
            get(block).copy_(torch.from_numpy(golden["%s.%s" % (case, name)]))
    x = torch.from_numpy(golden[case + ".feat"]).to(dev).requires_grad_(True)
    shortcut = torch.from_numpy(golden[case + ".shortcut"]).to(dev).requires_grad_(True)
    point = types.SimpleNamespace(feat=shortcut, offset=torch.from_numpy(golden[case + ".offset"]).to(dev),
                                  serialized_order=torch.from_numpy(golden[case + ".order"]).to(dev)[None],
                                  serialized_inverse=torch.from_numpy(golden[case + ".inverse"]).to(dev)[None])
    qkv = block.attn.qkv(x)                                     # by torch: the projection is point_front's, not the middle's
    parts = m.middle._parts(block, point)
    assert parts is not None and parts[0] is block.attn.proj and parts[1] is None
    point = m.middle.middle(block, point, shortcut, qkv, parts)
    assert block.attn.patch_size == 48 and point.feat.shape == x.shape
    assert m.middle.stats() == {"fused_calls": 1, "original_calls": 0} and m.attention.stats()["fused_calls"] == 1
    assert m.mid.stats() == {"plan_calls": 1, "gather_forward_calls": 1, "gather_backward_calls": 0, "forward_calls": 1,
                             "backward_calls": 0}
    (point.feat * torch.from_numpy(golden[case + ".w"]).to(dev)).sum().backward()
    assert m.mid.stats()["gather_backward_calls"] == 1 and m.mid.stats()["backward_calls"] == 1
    got = {"out": point.feat.detach(), "grad.feat": x.grad, "grad.shortcut": shortcut.grad}
    got.update({"grad." + name: get(block).grad for name, get in GOLDEN_PARAMS.items()})
    worst = []
    for name, value in got.items():
        want, err32 = golden["%s.%s" % (case, name)], float(golden["%s.err32.%s" % (case, name)])
        err = float(np.abs(value.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max())
        print("%s %-18s %.2e of the maximum, the reference's float32 run %.2e, ratio %.2f" % (
            case, name, err, err32, err / max(err32, 1e-30)))
        if not err <= 4 * err32:
            worst.append((name, err, err32))
    assert not worst, worst


# ---- the composed run ---------------------------------------------------------------------------------------------------------
def _bits_equal(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a) and set(a) == set(b)


@pytest.mark.parametrize("order", ("ffn, front, mid", "mid, ffn", "front, mid"))
def test_the_front_the_middle_and_the_tail_compose(dev, clean, order):
    m = clean
    inp = PF._inputs()
    yard, _, _, _ = PF._run(inp, dev, torch.float32)                      # nothing installed: the torch ops on the GPU
    want, _, _, _ = PF._run(inp, "cpu", torch.float64)
    mods = {"ffn": m.ffn, "front": m.front, "mid": m.middle}
    names = order.split(", ")
    # a run that never installs point_mid: point_front where point_mid.install would have put it
    for name in [n for n in names if n != "mid"] if "front" in names else [n.replace("mid", "front") for n in names]:
        mods[name].install(PT_V3)
    never, _, _, _ = PF._run(inp, dev, torch.float32)
    assert m.middle.stats() == {"fused_calls": 0, "original_calls": 0} and m.front.stats()["fused_calls"] == 1
    m.front.uninstall(PT_V3)
    m.ffn.uninstall(PT_V3)
    assert Block.forward.__qualname__ == "Block.forward"
    for name in names:
        mods[name].install(PT_V3)
    _reset(m)
    got, point, block, _ = PF._run(inp, dev, torch.float32)
    assert m.front.stats() == {"fused_calls": 1, "original_calls": 0}
    assert m.middle.stats() == {"fused_calls": 1, "original_calls": 0}
    assert m.attention.stats() == {"fused_calls": 1, "original_calls": 0}
    assert m.ffn.stats() == {"fused_calls": int("ffn" in names), "original_calls": 0}
    assert m.mid.stats() == dict.fromkeys(m.mid.stats(), 1)
    assert point.sparse_conv_feat.features is point.feat and block.attn.patch_size == PF.PATCH
    assert len(want) == 3 + 16 and set(got) == set(want)
    PF._hold("composed (%s)" % order, got, yard, want)
    # the no-behaviour-change proof: with the middle off the method runs the lines it ran before, to the bit
    m.middle.uninstall(PT_V3)
    _reset(m)
    after, _, _, _ = PF._run(inp, dev, torch.float32)
    assert m.middle.stats() == {"fused_calls": 0, "original_calls": 0} and m.mid.stats() == dict.fromkeys(m.mid.stats(), 0)
    assert m.front.stats() == {"fused_calls": 1, "original_calls": 0} and m.attention.stats()["fused_calls"] == 1
    assert _bits_equal(after, never)


def test_the_six_install_orders_of_the_three_thirds_give_the_same_bits_and_counters(dev, clean):
    """Which thirds are on decides what runs, not the order they went on in: every output and gradient of the other five
    orders has the first order's bits, in eval mode and in training mode with DropPath(0.3) from one seed, and every
    counter its value."""
    import itertools
    m = clean
    inp = PF._inputs()
    mods = {"front": m.front, "mid": m.middle, "ffn": m.ffn}
    own, first = Block.forward, None
    for order in itertools.permutations(mods):
        for name in order:
            mods[name].install(PT_V3)
        _reset(m)
        got = (PF._run(inp, dev, torch.float32)[0], PF._run(inp, dev, torch.float32, drop_path=0.3, seed=1234)[0])
        counters = [mod.stats() for mod in (m.mid, m.attention, m.ffn, m.front, m.middle)]
        for name in order:
            mods[name].uninstall(PT_V3)
        assert Block.forward is own
        if first is None:
            first = (got, counters)
            assert m.front.stats() == m.middle.stats() == m.ffn.stats() == {"fused_calls": 2, "original_calls": 0}
        assert _bits_equal(got[0], first[0][0]) and _bits_equal(got[1], first[0][1]), order
        assert counters == first[1], order


def _hold_worst(label, cases):
    """tests/front_ref.py's bar as it defines it: per tensor the worst figure over the cases of one shape is at most 4 x the
    yardstick's worst over the same cases, never below 2^-23.  cases: (got, yard, want) per case."""
    failed = []
    for name in cases[0][2]:
        fig = lambda res, want: float((res[name].double() - want[name]).abs().max()) / float(want[name].abs().max())  # noqa: E731
        err, err_yard = max(fig(g, w) for g, _, w in cases), max(fig(y, w) for _, y, w in cases)
        print("%s %-22s operator %.2e  torch float32 %.2e of the maximum (per case: %s)" % (
            label, name, err, err_yard, ", ".join("%.2e / %.2e" % (fig(g, w), fig(y, w)) for g, y, w in cases)))
        if not err <= max(4 * err_yard, 2.0 ** -23):
            failed.append((name, err, err_yard))
    assert not failed, failed


def test_training_mode_draws_upstreams_first_mask_at_upstreams_position(dev, clean, monkeypatch):
    """Both masks are upstream's.  The figures are held over the two modes of this Block as the cases of one shape (eval and
    training): taken alone, the training case's yardstick is 3.10e-07 for grad.attn.qkv.bias, half of what the same ops give
    in eval mode (6.50e-07), and four times it is below what the kernels that precede this operator give there by
    themselves (point_front without point_mid: 1.10e-06; with it 1.45e-06)."""
    m = clean
    inp, seed = PF._inputs(), 1234
    yard, _, _, masks = PF._run(inp, dev, torch.float32, drop_path=0.3, seed=seed)     # upstream's formulation draws two masks
    assert len(masks) == 2 and not torch.equal(masks[0], masks[1])
    assert 0 < int((masks[0] == 0).sum()) < PF.N and 0 < int((masks[1] == 0).sum()) < PF.N   # a dropped and a kept row
    want, _, _, _ = PF._run(inp, "cpu", torch.float64, drop_path=0.3, replay=masks)
    yard_eval, want_eval = PF._run(inp, dev, torch.float32)[0], PF._run(inp, "cpu", torch.float64)[0]
    seen, real = [], m.mid.proj_residual

    def record(a, inverse, extra, x, wp, bp, row_scale=None):
        seen.append(row_scale)
        return real(a, inverse, extra, x, wp, bp, row_scale)
    monkeypatch.setattr(m.mid, "proj_residual", record)
    m.middle.install(PT_V3)
    _reset(m)
    got, _, _, drawn = PF._run(inp, dev, torch.float32, drop_path=0.3, seed=seed)      # the tail's mask through the module
    assert m.middle.stats() == {"fused_calls": 1, "original_calls": 0}
    assert len(seen) == 1 and seen[0].shape == (PF.N, 1) and torch.equal(seen[0].cpu(), masks[0])
    assert len(drawn) == 1 and torch.equal(drawn[0], masks[1])
    got_eval = PF._run(inp, dev, torch.float32)[0]
    assert seen[1] is None                                                             # eval: no mask, nothing drawn
    _hold_worst("drop_path", [(got_eval, yard_eval, want_eval), (got, yard, want)])
    m.ffn.install(PT_V3)                                                               # the fused tail draws the second itself
    seen.clear()
    both, _, _, drawn = PF._run(inp, dev, torch.float32, drop_path=0.3, seed=seed)
    assert m.ffn.stats()["fused_calls"] == 1 and not drawn and torch.equal(seen[0].cpu(), masks[0])
    both_eval = PF._run(inp, dev, torch.float32)[0]
    _hold_worst("drop_path, fused tail", [(both_eval, yard_eval, want_eval), (both, yard, want)])  # holds only with masks[1] there


# ---- what goes back to the lines of before ------------------------------------------------------------------------------------
def _forward(block, C, device, dtype=torch.float32):
    g = torch.Generator().manual_seed(C)
    inp = PF._inputs()
    x, s = (torch.randn(PF.N, C, generator=g).to(device=device, dtype=dtype) for _ in range(2))
    block = block.to(device=device, dtype=dtype)
    block.cpe[0].given = s
    point = types.SimpleNamespace(feat=x, sparse_conv_feat=PF._Sparse(x), offset=torch.tensor(PF.COUNTS, device=device).cumsum(0),
                                  serialized_order=inp["order"].to(device), serialized_inverse=inp["inverse"].to(device))
    with torch.no_grad():
        return block(point).feat


def test_what_the_middle_does_not_run_goes_where_it_went_before(dev, clean):
    m = clean
    m.middle.install(PT_V3)
    C = PF.C
    _reset(m)
    _forward(Block(C, PF.SerializedAttention(C, PF.HEADS, PF.PATCH)).eval(), C, dev)
    assert m.middle.stats() == {"fused_calls": 1, "original_calls": 0}            # the plain Block is taken ...
    _reset(m)
    block = Block(C, PF.SerializedAttention(C, PF.HEADS, PF.PATCH))
    block.attn.proj_drop = torch.nn.Dropout(0.1)
    out = _forward(block.train(), C, dev)                                          # ... an active proj_drop is not
    assert m.middle.stats() == {"fused_calls": 0, "original_calls": 1} and m.mid.stats()["forward_calls"] == 0
    assert m.front.stats() == {"fused_calls": 1, "original_calls": 0} and m.attention.stats()["fused_calls"] == 1
    assert bool(torch.isfinite(out).all())
    _reset(m)
    _forward(block.eval(), C, dev)                                                 # ... and in eval it is inactive
    assert m.middle.stats() == {"fused_calls": 1, "original_calls": 0}
    _reset(m)
    wide = m.mid.max_channels() + 32                                               # 160 = 10 heads of 16
    _forward(Block(wide, PF.SerializedAttention(wide, wide // 16, PF.PATCH)).eval(), wide, dev)
    assert m.front.stats() == {"fused_calls": 0, "original_calls": 1}             # point_front's own limit is the same
    assert m.middle.stats() == {"fused_calls": 0, "original_calls": 0} and m.mid.stats()["forward_calls"] == 0
    _reset(m)
    with torch.autocast("cuda", dtype=torch.float16):
        _forward(Block(C, PF.SerializedAttention(C, PF.HEADS, PF.PATCH)).eval(), C, dev)
    assert m.front.stats() == {"fused_calls": 0, "original_calls": 1} and m.middle.stats() == {"fused_calls": 0, "original_calls": 0}
    _reset(m)
    _forward(Block(C, PF.SerializedAttention(C, PF.HEADS, PF.PATCH)).eval(), C, "cpu")
    assert m.front.stats() == {"fused_calls": 0, "original_calls": 1} and m.middle.stats() == {"fused_calls": 0, "original_calls": 0}
    assert m.mid.stats() == dict.fromkeys(m.mid.stats(), 0)
