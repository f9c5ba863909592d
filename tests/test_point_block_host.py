"""point_block, the one owner of Block.forward, without a GPU (not gpu): on tests/test_mid_host.py's stand-in models.pt_v3,
with the four fused bodies stubbed and the Block's own modules recording their names, point_front, point_mid and point_ffn go
on in each of their six orders and come off in each of the six.  After every step the record says which thirds are on, the
lines a Block reaches and the counters are those of that set alone -- for a Block every third accepts, for one the front
turns away and point_ffn takes (C = 256) and for CPU features -- and Block.forward is one object from the first bind to
the last unbind.  A foreign method bound over ours is left where it is."""
import itertools
import types

import pytest
import torch

from gaussiancity_amd import front, point_attention, point_block, point_ffn, point_front, point_mid
from test_mid_host import MINE, _FakeCuda, _marks, _stand_in

THIRDS = {"front": point_front, "mid": point_mid, "ffn": point_ffn}
ORDERS = [", ".join(p) for p in itertools.permutations(THIRDS)]
UPSTREAM_FRONT_AND_MIDDLE = ["cpe", "norm1", "attn", "drop_path"]
UPSTREAM_TAIL = ["norm2", "mlp", "drop_path"]


def lines(on):
    """What a Block that every third accepts reaches, by the thirds that are on (mid without front has no method to run in)."""
    if "front" not in on:
        return UPSTREAM_FRONT_AND_MIDDLE + ["point_ffn.fused_tail"] if "ffn" in on else [MINE]
    middle = ["point_mid.middle"] if "mid" in on else ["point_attention.forward_from_qkv", "drop_path"]
    return ["front.conv_tail_norm_qkv"] + middle + (["point_ffn.fused_tail"] if "ffn" in on else UPSTREAM_TAIL)


def wide_lines(on):
    """The same for a Block the front turns away and point_ffn takes."""
    return UPSTREAM_FRONT_AND_MIDDLE + ["point_ffn.fused_tail"] if "ffn" in on else [MINE]


class _Feat(_FakeCuda):
    def __add__(self, other):
        return self
    __radd__ = __add__


@pytest.fixture()
def world(monkeypatch):
    """(the stand-in, a function that resets the counters, runs a Block of width c and returns the names of what it reached)."""
    S, seen = _stand_in(), []

    def body(name, result):
        def stub(*args, **kwargs):
            seen.append(name)
            return result(*args)
        return stub
    monkeypatch.setattr(front, "conv_tail_norm_qkv", body("front.conv_tail_norm_qkv", lambda x, *rest: (x, "qkv")))
    monkeypatch.setattr(point_mid, "middle", body("point_mid.middle", lambda block, point, *rest: point))
    monkeypatch.setattr(point_attention, "forward_from_qkv", body("point_attention.forward_from_qkv", lambda attn, point, qkv: point))
    monkeypatch.setattr(point_ffn, "fused_tail", body("point_ffn.fused_tail", lambda point, *rest: point))
    blocks = {}

    def run(c, feat=None, block=None):
        if block is not None or c not in blocks:
            block = blocks[c] = S.Block(c=c) if block is None else block
            for name in ("cpe", "norm1", "attn", "norm2", "mlp", "drop_path"):  # upstream's lines, through the modules
                getattr(block, name).forward = body(name, lambda point: point)
            block.cpe[0].forward = lambda sparse: sparse
        sparse = types.SimpleNamespace(features=None)
        sparse.replace_feature = lambda f: sparse
        point = types.SimpleNamespace(feat=_Feat((5, c)) if feat is None else feat, sparse_conv_feat=sparse)
        del seen[:]
        for m in THIRDS.values():
            m.reset_stats()
        out = blocks[c](point)
        assert out is point or (out == MINE and not seen)
        return list(seen) if out is point else [MINE]
    return S, run


def _counters():
    return {name: m.stats() for name, m in THIRDS.items()}


def _check(S, run, on, own, bound):
    """Everything that must hold with the thirds `on` on, whatever came before; returns the bound method."""
    st = point_block.state(S)
    if not on:
        assert st is None and not _marks(S) and S.Block.forward is own
        return bound
    assert _marks(S) == [point_block._STATE]
    assert (st.front is not None, st.mid, st.ffn is not None) == ("front" in on, "mid" in on, "ffn" in on)
    if on <= {"mid"}:
        assert S.Block.forward is own and st.bound is None and st.original is None
    else:
        bound = S.Block.forward if bound is None else bound
        assert S.Block.forward is bound and bound is not own and st.bound is bound and st.original is own
    took = int("front" in on)
    assert run(16) == lines(on), on
    assert _counters() == {"front": {"fused_calls": took, "original_calls": 0}, "mid": {"fused_calls": 0, "original_calls": 0},
                           "ffn": {"fused_calls": 0, "original_calls": 0}}, on
    assert run(256) == wide_lines(on), on                                   # the front turns it away, point_ffn takes it
    assert _counters() == {"front": {"fused_calls": 0, "original_calls": took}, "mid": {"fused_calls": 0, "original_calls": 0},
                           "ffn": {"fused_calls": 0, "original_calls": 0}}, on
    assert run(16, torch.randn(5, 16)) == [MINE]                            # CPU features: every third that is on turns it away
    assert _counters() == {"front": {"fused_calls": 0, "original_calls": took}, "mid": {"fused_calls": 0, "original_calls": 0},
                           "ffn": {"fused_calls": 0, "original_calls": int("ffn" in on)}}, on
    return bound


@pytest.mark.parametrize("uninstall_order", ORDERS)
@pytest.mark.parametrize("install_order", ORDERS)
def test_what_runs_is_a_function_of_the_thirds_that_are_on(world, install_order, uninstall_order):
    S, run = world
    own, on = S.Block.forward, set()
    bound = _check(S, run, on, own, None)
    for name in install_order.split(", "):
        THIRDS[name].install(S, **({"max_channels": 512} if name == "ffn" else {}))
        on |= {name, "front"} if name == "mid" else {name}                  # point_mid turns the front on when it is off
        bound = _check(S, run, on, own, bound)
    assert on == set(THIRDS) and point_block.state(S).ffn == (512, False)
    for name in uninstall_order.split(", "):
        THIRDS[name].uninstall(S)
        on -= {name}
        bound = _check(S, run, on, own, bound)
    assert S.Block.forward is own and not _marks(S)


def test_the_fronts_count_of_the_blocks_it_turns_away_does_not_depend_on_the_install_order(world):
    S, run = world
    for order in (("ffn", "front"), ("front", "ffn")):
        for name in order:
            THIRDS[name].install(S, **({"max_channels": 512} if name == "ffn" else {}))
        assert run(256) == wide_lines({"front", "ffn"})
        assert point_front.stats() == {"fused_calls": 0, "original_calls": 1}, order
        assert point_ffn.stats() == {"fused_calls": 0, "original_calls": 0}, order     # it took the Block (the stub counts nothing)
        for name in order:
            THIRDS[name].uninstall(S)
        assert point_block.state(S) is None


def test_a_block_the_middle_turns_away_runs_the_fronts_own_lines_and_is_counted(world):
    S, run = world
    point_mid.install(S)
    point_ffn.install(S)
    active = S.Block(attn=S.Attn(16, proj_drop=0.1)).train()                # an active proj_drop: not the fused middle's
    assert run(16, block=active) == lines({"front", "ffn"})
    assert _counters() == {"front": {"fused_calls": 1, "original_calls": 0}, "mid": {"fused_calls": 0, "original_calls": 1},
                           "ffn": {"fused_calls": 0, "original_calls": 0}}
    assert run(16, block=active.eval()) == lines({"front", "mid", "ffn"})
    assert point_mid.stats() == {"fused_calls": 0, "original_calls": 0}     # taken (the stub counts nothing)
    for m in THIRDS.values():
        m.uninstall(S)
    assert not _marks(S)


def test_an_install_that_raises_changes_nothing(world):
    S, run = world
    point_mid.install(S)
    point_ffn.install(S, max_channels=256, split=True)
    st = point_block.state(S)
    before = (S.Block.forward, st.original, st.bound, st.front, st.mid, st.ffn)
    for install, kwargs in ((point_ffn.install, {"max_channels": 516}), (point_ffn.install, {"split": 1}),
                            (point_front.install, {"max_channels": -4}), (point_front.install, {"max_channels": 2.5})):
        with pytest.raises(ValueError):
            install(S, **kwargs)
        assert point_block.state(S) is st and (S.Block.forward, st.original, st.bound, st.front, st.mid, st.ffn) == before
    point_ffn.install(S, max_channels=512)                                   # a repeated install takes over new keyword values
    point_front.install(S, max_channels=64)
    point_mid.install(S)                                                     # ... and point_mid leaves a cap that is set
    assert (S.Block.forward, st.front, st.mid, st.ffn) == (before[0], 64, True, (512, False))
    for m in THIRDS.values():
        m.uninstall(S)
    assert not _marks(S)


@pytest.mark.parametrize("mid_on", (False, True))
def test_a_foreign_method_bound_over_ours_is_left_alone(world, mid_on):
    S, run = world
    own = S.Block.forward
    (point_mid if mid_on else point_front).install(S)
    point_ffn.install(S)
    ours = S.Block.forward

    def foreign(self, point):
        return ours(self, point)
    S.Block.forward = foreign
    assert run(16) == lines({"front", "ffn"} | ({"mid"} if mid_on else set()))  # through the foreign method, ours still runs
    point_ffn.uninstall(S)
    assert S.Block.forward is foreign and point_block.state(S).bound is ours    # the front is on: nothing to put back yet
    point_front.uninstall(S)
    st = point_block.state(S)
    assert S.Block.forward is foreign                                       # not ours to put back
    assert (st is not None and (st.original, st.bound, st.front, st.mid, st.ffn) == (None, None, None, True, None)) if mid_on else st is None
    assert run(16) == [MINE] and run(256) == [MINE]                         # ours finds no record of itself: the method it found
    assert _counters() == dict.fromkeys(THIRDS, {"fused_calls": 0, "original_calls": 0})
    point_front.install(S)                                                  # binds again, over the foreign method
    again = S.Block.forward
    assert again is not ours and again is not foreign and point_block.state(S).original is foreign
    assert run(16) == lines({"front", "mid"} if mid_on else {"front"})
    point_front.uninstall(S)
    point_mid.uninstall(S)
    assert S.Block.forward is foreign and not _marks(S)
    S.Block.forward = own
