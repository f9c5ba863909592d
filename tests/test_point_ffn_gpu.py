"""-m gpu: point_ffn's rebound Block.forward against the reference's own modules (tests/golden/ptv3_block_ffn.npz, written
by tests/golden/make_ptv3_block_ffn_golden.py from models/pt_v3.py's LayerNorm + MLP + residual in float64, with the error
of the reference's own float32 run per tensor).  The Block here is a stand-in whose own forward raises: it holds its
sub-modules under upstream's names, cpe / norm1 / attn are recording identities.  Identities double the features twice
(two residual adds), so the Block is fed feat / 4 -- exact in binary -- and the tail sees the fixture's feat.

Every output and gradient is within 4 x err32 of the fixture (the scheme and the margin of the other backbone bindings).
In training mode with DropPath(0.3) the rebound method draws the same masks as upstream's formulation run from the same
seed: the dropped rows are the same set and bit-equal to the shortcut, the rest meets test_ffn_gpu.py's bar against the
same formulation in float64 (4 x the figure of the torch float32 run on the GPU, never below 2^-23)."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ptv3_block_ffn.npz"))


# ---- what install() needs of models/pt_v3.py, written for this test -------------------------------------------------------
class _Sparse:
    def __init__(self, features):
        self.features = features

    def replace_feature(self, features):
        return _Sparse(features)


class _Seq(torch.nn.Module):
    """PointSequential for plain torch modules: each one maps point.feat."""
    def __init__(self, *mods):
        super().__init__()
        for i, m in enumerate(mods):
            self.add_module(str(i), m)

    def __getitem__(self, i):
        return list(self._modules.values())[i]

    def forward(self, point):
        for m in self._modules.values():
            point.feat = m(point.feat)
        return point


class _Recorder(torch.nn.Module):
    """An identity on the point that writes its name into the Block's log."""
    def __init__(self, name, log):
        super().__init__()
        self.name, self.log = name, log

    def forward(self, point):
        self.log.append(self.name)
        return point


class _DropPath(torch.nn.Module):
    """DropPath of models/pt_v3.py by its behaviour: one bernoulli draw per row, scaled by 1 / keep."""
    def __init__(self, drop_prob, scale_by_keep=True):
        super().__init__()
        self.drop_prob, self.scale_by_keep, self.masks = drop_prob, scale_by_keep, []

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep)
        if keep > 0.0 and self.scale_by_keep:
            mask.div_(keep)
        self.masks.append(mask)
        return x * mask


class _MLP(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.fc1, self.act, self.fc2 = torch.nn.Linear(c, 4 * c), torch.nn.GELU(), torch.nn.Linear(4 * c, c)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class Block(torch.nn.Module):
    def __init__(self, c, drop_path=0.0):
        super().__init__()
        self.pre_norm, self.log = True, []
        self.cpe, self.norm1, self.attn = (_Recorder(n, self.log) for n in ("cpe", "norm1", "attn"))
        self.norm2, self.mlp = _Seq(torch.nn.LayerNorm(c)), _Seq(_MLP(c))
        self.drop_path = _Seq(_DropPath(drop_path) if drop_path > 0.0 else torch.nn.Identity())

    def forward(self, point):
        raise AssertionError("the stand-in Block does not compute: the rebound method must")

    def named(self):
        return {"norm.weight": self.norm2[0].weight, "norm.bias": self.norm2[0].bias, "fc1.weight": self.mlp[0].fc1.weight,
                "fc1.bias": self.mlp[0].fc1.bias, "fc2.weight": self.mlp[0].fc2.weight, "fc2.bias": self.mlp[0].fc2.bias}


def upstream_forward(self, point):
    """Block.forward of models/pt_v3.py (pre_norm) by its behaviour, over the modules themselves."""
    shortcut = point.feat
    point = self.cpe(point)
    point.feat = shortcut + point.feat
    shortcut = point.feat
    point = self.norm1(point)
    point = self.drop_path(self.attn(point))
    point.feat = shortcut + point.feat
    shortcut = point.feat
    point = self.norm2(point)
    point = self.drop_path(self.mlp(point))
    point.feat = shortcut + point.feat
    point.sparse_conv_feat = point.sparse_conv_feat.replace_feature(point.feat)
    return point


@pytest.fixture()
def bound():
    from gaussiancity_amd import point_ffn
    P = types.SimpleNamespace(Block=Block)
    own = Block.forward
    point_ffn.install(P)
    point_ffn.reset_stats()
    yield point_ffn
    point_ffn.uninstall(P)
    assert Block.forward is own


def _block(golden, case, device, dtype=torch.float32, drop_path=0.0):
    C = golden[case + ".feat"].shape[1]
    block = Block(C, drop_path).to(device=device, dtype=dtype)
    with torch.no_grad():
        for name, p in block.named().items():
            p.copy_(torch.from_numpy(golden["%s.%s" % (case, name)]).to(dtype))
    assert block.norm2[0].eps == float(golden[case + ".eps"])
    return block


def _point(feat):
    return types.SimpleNamespace(feat=feat, sparse_conv_feat=_Sparse(feat))


@pytest.mark.parametrize("case", ["c32", "c64"])
def test_rebound_block_matches_the_reference_run(dev, bound, golden, case):
    block = _block(golden, case, dev)
    x = (torch.from_numpy(golden[case + ".feat"]) / 4).to(dev).requires_grad_(True)
    point = block(_point(x))
    assert bound.stats() == {"fused_calls": 1, "original_calls": 0} and block.log == ["cpe", "norm1", "attn"]
    assert point.sparse_conv_feat.features is point.feat and point.feat.shape == x.shape
    (point.feat * torch.from_numpy(golden[case + ".w"]).to(dev)).sum().backward()
    got = {"out": point.feat.detach(), "grad.feat": x.grad / 4}
    got.update({"grad." + name: p.grad for name, p in block.named().items()})
    worst = []
    for name, value in got.items():
        want, err32 = golden["%s.%s" % (case, name)], float(golden["%s.err32.%s" % (case, name)])
        err = float(np.abs(value.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max())
        print("%s %-18s %.2e of the maximum, the reference's float32 run %.2e" % (case, name, err, err32))
        if not err <= 4 * err32:
            worst.append((name, err, err32))
    assert not worst, worst


def test_training_mode_draws_upstreams_masks_and_drops_the_same_rows(dev, bound, golden):
    case, seed = "c32", 1234
    feat, w = torch.from_numpy(golden[case + ".feat"]) / 4, torch.from_numpy(golden[case + ".w"])

    def run(forward, device, dtype, masks=None):
        block = _block(golden, case, device, dtype, drop_path=0.3).train()
        drop = block.drop_path[0]
        if masks is not None:   # the float64 target replays the masks the GPU drew
            replay = iter(masks)
            drop.forward = lambda t: t * next(replay).to(device=t.device, dtype=t.dtype)
        x = feat.to(device=device, dtype=dtype).requires_grad_(True)
        torch.manual_seed(seed)
        point = forward(block, _point(x))
        (point.feat * w.to(device=device, dtype=dtype)).sum().backward()
        res = {"out": point.feat.detach().cpu(), "grad.feat": x.grad.cpu()}
        res.update({"grad." + n: p.grad.cpu() for n, p in block.named().items()})
        return res, [m.cpu() for m in drop.masks], point

    yard, masks, _ = run(upstream_forward, dev, torch.float32)
    assert len(masks) == 2 and bound.stats()["fused_calls"] == 0
    got, first, point = run(lambda b, p: b(p), dev, torch.float32)      # the rebound method
    assert bound.stats() == {"fused_calls": 1, "original_calls": 0}
    assert len(first) == 1 and torch.equal(first[0], masks[0])            # the attention branch's mask, drawn first
    assert point.sparse_conv_feat.features is point.feat
    want, _, _ = run(upstream_forward, "cpu", torch.float64, masks)

    # the tail's shortcut: feat / 4, doubled, then plus the first mask times itself -- the same bits on every path
    u = 2 * feat
    shortcut = u + u * masks[0]
    dropped = masks[1][:, 0] == 0
    assert 0 < int(dropped.sum()) < len(dropped)
    view = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    assert torch.equal(view(got["out"][dropped]), view(shortcut[dropped]))
    assert torch.equal(view(yard["out"][dropped]), view(shortcut[dropped]))
    moved = (got["out"] != shortcut).any(dim=1)
    assert torch.equal(moved, ~dropped)                                     # the same set of rows, no more and no fewer
    failed = []
    for name in want:
        top = float(want[name].abs().max())
        err = float((got[name].double() - want[name]).abs().max()) / top
        err_yard = float((yard[name].double() - want[name]).abs().max()) / top
        print("drop_path %-18s operator %.2e  torch float32 %.2e of the maximum" % (name, err, err_yard))
        if not err <= max(4 * err_yard, 2.0 ** -23):
            failed.append((name, err, err_yard))
    assert not failed, failed
