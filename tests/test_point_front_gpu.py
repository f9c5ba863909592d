"""-m gpu: point_front's rebound Block.forward.

Golden.  Against the reference's own modules (tests/golden/ptv3_block_front.npz, written by
tests/golden/make_ptv3_block_front_golden.py from models/pt_v3.py's PointSequential(Linear, LayerNorm), residual add,
PointSequential(LayerNorm) and SerializedAttention.qkv in float64, with the error of the reference's own float32 run per
tensor).  The Block is a stand-in: cpe[0] is a stand-in spconv module that returns the fixture's convolution output, the
attention is recorded where point_front hands it the projection (point_attention.forward_from_qkv) and contributes zeros,
norm2 and mlp are identities, so the Block's output is 2 x feat -- exact in binary.  Every output and gradient is within
4 x err32 of the fixture (the scheme and the margin of the other backbone bindings).

Composed.  The real point_attention path and point_ffn's fused tail on a stand-in Block with a real attention module, two
batch elements and a patch size below the smaller one, against upstream's formulation written by its behaviour: float64 on
the CPU as target, float32 on the GPU with nothing installed as yardstick, and test_front_gpu.py's bar (4 x the yardstick's
figure, never below 2^-23).  In training mode with DropPath(0.3) the rebound method draws upstream's two masks from the same
seed in the same order.  Nothing here reads the reference: the fixture and the stand-ins only."""
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
    from gaussiancity_amd import _native_a, _native_m
    _native_m.lib()
    _native_a.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ptv3_block_front.npz"))


# ---- what install() needs of models/pt_v3.py, written for this test by the behaviour of its classes ---------------------------
class _Sparse:
    def __init__(self, features):
        self.features = features

    def replace_feature(self, features):
        return _Sparse(features)


class _Conv(torch.nn.Module):
    """The sparse convolution's stand-in: whatever comes in, its output features are the tensor it was given."""
    def __init__(self):
        super().__init__()
        self.given = None

    def forward(self, sparse):
        return _Sparse(self.given)


class _Seq(torch.nn.Module):
    """PointSequential: a spconv module maps point.sparse_conv_feat and point.feat follows, a torch module maps point.feat
    and sparse_conv_feat follows."""
    def __init__(self, *mods):
        super().__init__()
        for i, m in enumerate(mods):
            self.add_module(str(i), m)

    def __getitem__(self, i):
        return list(self._modules.values())[i]

    def forward(self, point):
        for m in self._modules.values():
            if isinstance(m, _Conv):
                point.sparse_conv_feat = m(point.sparse_conv_feat)
                point.feat = point.sparse_conv_feat.features
            else:
                point.feat = m(point.feat)
                point.sparse_conv_feat = point.sparse_conv_feat.replace_feature(point.feat)
        return point


class _DropPath(torch.nn.Module):
    """DropPath by its behaviour: one bernoulli draw per row, scaled by 1 / keep.  replay: masks to use instead of drawing."""
    def __init__(self, drop_prob, scale_by_keep=True):
        super().__init__()
        self.drop_prob, self.scale_by_keep, self.masks, self.replay = drop_prob, scale_by_keep, [], None

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        if self.replay is not None:
            return x * self.replay.pop(0).to(device=x.device, dtype=x.dtype)
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


class _PointIdentity(torch.nn.Module):
    def forward(self, point):
        return point


class SerializedAttention(torch.nn.Module):
    """SerializedAttention (non-flash) by its behaviour: the patch size is the smallest batch element's count, capped;
    the points go in serialized order into patches of that size, a batch element's last patch filled up from the one
    before; softmax(q scale k^T) v per patch and head; back in point order through the projection."""
    def __init__(self, channels, num_heads, patch_size):
        super().__init__()
        self.channels, self.num_heads, self.scale, self.order_index = channels, num_heads, (channels // num_heads) ** -0.5, 0
        self.enable_flash = self.enable_rpe = False
        self.patch_size_max, self.patch_size = patch_size, 0
        self.attn_drop, self.proj_drop = torch.nn.Dropout(0.0), torch.nn.Dropout(0.0)
        self.qkv, self.proj = torch.nn.Linear(channels, channels * 3), torch.nn.Linear(channels, channels)

    def get_padding_and_inverse(self, point):
        K, pad, unpad, cu, start, pstart = self.patch_size, [], [], [0], 0, 0
        for end in point.offset.tolist():
            n = end - start
            own = list(range(n))
            if n > K and n % K:                       # the last patch: its own n % K points, then the rest of the one before
                m, r = n // K, n % K
                own += list(range((m - 1) * K + r, m * K))
            pad += [start + j for j in own]
            unpad += [pstart + j for j in range(n)]
            cu += [pstart + k for k in range(K, len(own) + 1, K)] if n >= K else [pstart + n]
            start, pstart = end, pstart + len(own)
        dev = point.offset.device
        return (torch.tensor(pad, device=dev), torch.tensor(unpad, device=dev), torch.tensor(cu, dtype=torch.int32, device=dev))

    def forward(self, point):
        counts = torch.diff(point.offset, prepend=point.offset.new_zeros(1))
        self.patch_size = K = min(int(counts.min()), self.patch_size_max)
        H, C = self.num_heads, self.channels
        pad, unpad, _ = self.get_padding_and_inverse(point)
        order = point.serialized_order[self.order_index][pad]
        inverse = unpad[point.serialized_inverse[self.order_index]]
        q, k, v = self.qkv(point.feat)[order].reshape(-1, K, 3, H, C // H).permute(2, 0, 3, 1, 4).unbind(dim=0)
        attn = torch.softmax((q * self.scale) @ k.transpose(-2, -1), dim=-1)
        feat = (attn @ v).transpose(1, 2).reshape(-1, C)[inverse]
        point.feat = self.proj_drop(self.proj(feat))
        return point


class Block(torch.nn.Module):
    """Block (pre_norm) by its behaviour: the order of its modules, of its residual adds and of the DropPath draws."""
    def __init__(self, c, attn, drop_path=0.0, tail=True):
        super().__init__()
        self.pre_norm = True
        self.cpe = _Seq(_Conv(), torch.nn.Linear(c, c), torch.nn.LayerNorm(c))
        self.norm1, self.attn = _Seq(torch.nn.LayerNorm(c)), attn
        self.norm2 = _Seq(torch.nn.LayerNorm(c)) if tail else _PointIdentity()
        self.mlp = _Seq(_MLP(c)) if tail else _PointIdentity()
        self.drop_path = _Seq(_DropPath(drop_path) if drop_path > 0.0 else torch.nn.Identity())

    def forward(self, point):
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


PT_V3 = types.SimpleNamespace(Block=Block, spconv=types.SimpleNamespace(
    modules=types.SimpleNamespace(is_spconv_module=lambda m: isinstance(m, _Conv))))


@pytest.fixture()
def installed():
    """point_front alone; a test adds point_ffn itself.  Everything is taken off again."""
    from gaussiancity_amd import point_attention, point_ffn, point_front
    own = Block.forward
    point_front.install(PT_V3)
    for m in (point_front, point_ffn, point_attention):
        m.reset_stats()
    yield point_front, point_ffn, point_attention
    point_front.uninstall(PT_V3)
    point_ffn.uninstall(PT_V3)
    assert Block.forward is own and not [n for n in vars(PT_V3) if n.startswith("_gaussiancity_amd")]


# ---- the golden run ---------------------------------------------------------------------------------------------------------
class _QkvOnly(torch.nn.Module):
    """What point_front reads of the attention before it hands over the projection."""
    def __init__(self, c):
        super().__init__()
        self.channels, self.num_heads, self.enable_flash, self.enable_rpe = c, c // 16, False, False
        self.attn_drop, self.qkv = torch.nn.Dropout(0.0), torch.nn.Linear(c, 3 * c)

    def forward(self, point):
        raise AssertionError("the attention's own forward ran: point_front hands the projection to forward_from_qkv")


GOLDEN_PARAMS = {"cpe.1.weight": lambda b: b.cpe[1].weight, "cpe.1.bias": lambda b: b.cpe[1].bias,
                 "cpe.2.weight": lambda b: b.cpe[2].weight, "cpe.2.bias": lambda b: b.cpe[2].bias,
                 "norm1.weight": lambda b: b.norm1[0].weight, "norm1.bias": lambda b: b.norm1[0].bias,
                 "qkv.weight": lambda b: b.attn.qkv.weight, "qkv.bias": lambda b: b.attn.qkv.bias}


@pytest.mark.parametrize("case", ["c32", "c64"])
def test_rebound_block_matches_the_reference_run(dev, installed, golden, case, monkeypatch):
    point_front, _, point_attention = installed
    C = golden[case + ".feat"].shape[1]
    block = Block(C, _QkvOnly(C), tail=False).to(dev)
    with torch.no_grad():
        for name, get in GOLDEN_PARAMS.items():
            get(block).copy_(torch.from_numpy(golden["%s.%s" % (case, name)]))
    assert block.cpe[2].eps == float(golden[case + ".eps.cpe"]) and block.norm1[0].eps == float(golden[case + ".eps.norm1"])
    x = torch.from_numpy(golden[case + ".feat"]).to(dev).requires_grad_(True)
    s = torch.from_numpy(golden[case + ".conv"]).to(dev).requires_grad_(True)
    block.cpe[0].given = s
    seen = []

    def record(attn, point, qkv):
        seen.append((attn, point.feat, qkv))
        point.feat = torch.zeros_like(point.feat)
        return point
    monkeypatch.setattr(point_attention, "forward_from_qkv", record)
    point = block(types.SimpleNamespace(feat=x, sparse_conv_feat=_Sparse(x)))
    assert point_front.stats() == {"fused_calls": 1, "original_calls": 0} and len(seen) == 1 and seen[0][0] is block.attn
    assert point.sparse_conv_feat.features is point.feat and point.feat.shape == x.shape
    feat, qkv = seen[0][1], seen[0][2]
    assert torch.equal(point.feat.detach(), 2 * feat.detach())             # feat + 0, then twice itself through the identities
    w = lambda k: torch.from_numpy(golden["%s.w.%s" % (case, k)]).to(dev)  # noqa: E731
    ((point.feat / 2 * w("feat")).sum() + (qkv * w("qkv")).sum()).backward()
    got = {"out.feat": feat.detach(), "out.qkv": qkv.detach(), "grad.feat": x.grad, "grad.conv": s.grad}
    got.update({"grad." + name: get(block).grad for name, get in GOLDEN_PARAMS.items()})
    worst = []
    for name, value in got.items():
        want, err32 = golden["%s.%s" % (case, name)], float(golden["%s.err32.%s" % (case, name)])
        err = float(np.abs(value.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max())
        print("%s %-18s %.2e of the maximum, the reference's float32 run %.2e" % (case, name, err, err32))
        if not err <= 4 * err32:
            worst.append((name, err, err32))
    assert not worst, worst


# ---- the composed run ---------------------------------------------------------------------------------------------------------
N, C, HEADS, PATCH, COUNTS = 150, 32, 2, 48, (90, 60)   # two batch elements, both above the patch size, neither a multiple


def _inputs():
    g = torch.Generator().manual_seed(20261020)
    block = Block(C, SerializedAttention(C, HEADS, PATCH))
    with torch.no_grad():
        for p in block.parameters():                      # every parameter seeded, the LayerNorms away from (1, 0)
            p.copy_(torch.randn(p.shape, generator=g) * (p.shape[-1] ** -0.5 if p.dim() == 2 else 0.1) + (p.dim() == 1))
    order = torch.cat([torch.randperm(n, generator=g) + o for n, o in zip(COUNTS, (0, COUNTS[0]))])
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(N)
    return {"state": block.state_dict(), "x": torch.randn(N, C, generator=g), "s": torch.randn(N, C, generator=g),
            "w": torch.randn(N, C, generator=g), "order": order[None], "inverse": inverse[None]}


def _run(inp, device, dtype, drop_path=0.0, seed=None, replay=None):
    """One forward and backward of Block(...)(point) -- whatever is bound -- with the loss (out * w).sum()."""
    block = Block(C, SerializedAttention(C, HEADS, PATCH), drop_path)
    block.load_state_dict(inp["state"])
    block = block.to(device=device, dtype=dtype).train(drop_path > 0.0)
    drop = block.drop_path[0]
    if replay is not None:
        drop.replay = list(replay)
    x, s = (inp[k].detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for k in ("x", "s"))
    block.cpe[0].given = s
    point = types.SimpleNamespace(feat=x, sparse_conv_feat=_Sparse(x), offset=torch.tensor(COUNTS, device=device).cumsum(0),
                                  serialized_order=inp["order"].to(device), serialized_inverse=inp["inverse"].to(device))
    if seed is not None:
        torch.manual_seed(seed)
    point = block(point)
    (point.feat * inp["w"].to(device=device, dtype=dtype)).sum().backward()
    res = {"out": point.feat.detach(), "grad.x": x.grad, "grad.s": s.grad}
    res.update({"grad." + n: p.grad for n, p in block.named_parameters()})
    return {k: v.detach().cpu() for k, v in res.items()}, point, block, [m.cpu() for m in getattr(drop, "masks", [])]


def _hold(label, got, yard, want):
    failed = []
    for name in want:
        top = float(want[name].abs().max())
        err = float((got[name].double() - want[name]).abs().max()) / top
        err_yard = float((yard[name].double() - want[name]).abs().max()) / top
        print("%s %-22s operator %.2e  torch float32 %.2e of the maximum" % (label, name, err, err_yard))
        if not err <= max(4 * err_yard, 2.0 ** -23):
            failed.append((name, err, err_yard))
    assert not failed, failed


def test_the_front_the_attention_and_the_tail_compose(dev, installed):
    point_front, point_ffn, point_attention = installed
    inp = _inputs()
    point_front.uninstall(PT_V3)
    own = Block.forward
    assert own.__qualname__ == "Block.forward"
    yard, _, _, _ = _run(inp, dev, torch.float32)                        # nothing installed: the torch ops on the GPU
    want, _, _, _ = _run(inp, "cpu", torch.float64)
    point_ffn.install(PT_V3)
    point_front.install(PT_V3)
    for m in (point_front, point_ffn, point_attention):
        m.reset_stats()
    got, point, block, _ = _run(inp, dev, torch.float32)
    assert point_front.stats() == {"fused_calls": 1, "original_calls": 0}
    assert point_ffn.stats() == {"fused_calls": 1, "original_calls": 0}
    assert point_attention.stats() == {"fused_calls": 1, "original_calls": 0}
    assert point.sparse_conv_feat.features is point.feat and block.attn.patch_size == PATCH
    assert len(want) == 3 + 16 and set(got) == set(want)
    _hold("composed", got, yard, want)
    # the other install order: the same thirds are on, so the same lines run
    point_front.uninstall(PT_V3)
    point_ffn.uninstall(PT_V3)
    assert Block.forward is own
    point_front.install(PT_V3)
    point_ffn.install(PT_V3)
    for m in (point_front, point_ffn, point_attention):
        m.reset_stats()
    again, _, _, _ = _run(inp, dev, torch.float32)
    assert point_front.stats()["fused_calls"] == 1 and point_ffn.stats() == {"fused_calls": 1, "original_calls": 0}
    assert all(torch.equal(again[k].view(torch.int32), got[k].view(torch.int32)) for k in got)


def test_training_mode_draws_upstreams_masks_in_upstreams_order(dev, installed):
    point_front, point_ffn, _ = installed
    inp, seed = _inputs(), 1234
    point_front.uninstall(PT_V3)
    yard, _, _, masks = _run(inp, dev, torch.float32, drop_path=0.3, seed=seed)    # upstream's formulation draws two masks
    assert len(masks) == 2 and not torch.equal(masks[0], masks[1]) and all(0 < int((m == 0).sum()) < N for m in masks)
    want, _, _, _ = _run(inp, "cpu", torch.float64, drop_path=0.3, replay=masks)
    point_front.install(PT_V3)
    point_front.reset_stats()
    got, _, _, drawn = _run(inp, dev, torch.float32, drop_path=0.3, seed=seed)     # the tail through the modules: both recorded
    assert point_front.stats() == {"fused_calls": 1, "original_calls": 0}
    assert len(drawn) == 2 and torch.equal(drawn[0], masks[0]) and torch.equal(drawn[1], masks[1])
    _hold("drop_path", got, yard, want)
    point_ffn.install(PT_V3)                                                       # the fused tail draws the second itself
    both, _, _, drawn = _run(inp, dev, torch.float32, drop_path=0.3, seed=seed)
    assert point_ffn.stats()["fused_calls"] == 1 and len(drawn) == 1 and torch.equal(drawn[0], masks[0])
    _hold("drop_path, fused tail", both, yard, want)
