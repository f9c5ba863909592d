"""-m gpu: point_ffn.install(..., max_channels=512) on Blocks wider than the one-launch kernels hold, after
tests/test_point_ffn_gpu.py (whose stand-in modules and upstream formulation are used here).

Against the reference's own modules (tests/golden/ptv3_block_ffn_wide.npz, written by
tests/golden/make_ptv3_block_ffn_wide_golden.py: 65 rows, C = 132, MLP(hidden_channels=72), float64 with the error of the
reference's float32 run per tensor): every output and gradient is within 4 x err32, never below 2^-23, and the split path
was taken.  In training mode at C = 256 with DropPath(0.3) the rebound method draws upstream's masks from the same seed,
drops the same rows (bit-equal to the shortcut) and meets tests/ffn_ref.py's bar on the rest."""
import os
import types

import numpy as np
import pytest
import torch

from test_point_ffn_gpu import _DropPath, _point, _Recorder, _Seq, upstream_forward

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("norm.weight", "norm.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


class _MLP(torch.nn.Module):
    def __init__(self, c, hidden):
        super().__init__()
        self.fc1, self.act, self.fc2 = torch.nn.Linear(c, hidden), torch.nn.GELU(), torch.nn.Linear(hidden, c)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class Block(torch.nn.Module):
    """tests/test_point_ffn_gpu.py's stand-in with a hidden width of its own."""
    def __init__(self, c, hidden, drop_path=0.0):
        super().__init__()
        self.pre_norm, self.log = True, []
        self.cpe, self.norm1, self.attn = (_Recorder(n, self.log) for n in ("cpe", "norm1", "attn"))
        self.norm2, self.mlp = _Seq(torch.nn.LayerNorm(c)), _Seq(_MLP(c, hidden))
        self.drop_path = _Seq(_DropPath(drop_path) if drop_path > 0.0 else torch.nn.Identity())

    def forward(self, point):
        raise AssertionError("the stand-in Block does not compute: the rebound method must")

    def named(self):
        return {"norm.weight": self.norm2[0].weight, "norm.bias": self.norm2[0].bias, "fc1.weight": self.mlp[0].fc1.weight,
                "fc1.bias": self.mlp[0].fc1.bias, "fc2.weight": self.mlp[0].fc2.weight, "fc2.bias": self.mlp[0].fc2.bias}


@pytest.fixture()
def bound():
    from gaussiancity_amd import point_ffn
    P = types.SimpleNamespace(Block=Block)
    own = Block.forward
    point_ffn.install(P, max_channels=512)
    point_ffn.reset_stats()
    yield point_ffn
    point_ffn.uninstall(P)
    assert Block.forward is own


def _block(params, device, dtype=torch.float32, drop_path=0.0):
    hidden, c = params["fc1.weight"].shape
    block = Block(c, hidden, drop_path).to(device=device, dtype=dtype)
    with torch.no_grad():
        for name, p in block.named().items():
            p.copy_(torch.as_tensor(params[name]).to(dtype))
    return block


def test_rebound_wide_block_matches_the_reference_run(dev, bound):
    golden, case = np.load(os.path.join(ROOT, "tests", "golden", "ptv3_block_ffn_wide.npz")), "c132"
    block = _block({n: golden["%s.%s" % (case, n)] for n in NAMES}, dev)
    assert block.norm2[0].eps == float(golden[case + ".eps"]) and golden[case + ".feat"].shape == (65, 132)
    x = (torch.from_numpy(golden[case + ".feat"]) / 4).to(dev).requires_grad_(True)
    point = block(_point(x))
    assert bound.stats() == {"fused_calls": 1, "original_calls": 0} and block.log == ["cpe", "norm1", "attn"]
    assert bound.split_stats() == {"fused_calls": 1}
    assert point.sparse_conv_feat.features is point.feat and point.feat.shape == x.shape
    (point.feat * torch.from_numpy(golden[case + ".w"]).to(dev)).sum().backward()
    got = {"out": point.feat.detach(), "grad.feat": x.grad / 4}
    got.update({"grad." + name: p.grad for name, p in block.named().items()})
    worst = []
    for name, value in got.items():
        want, err32 = golden["%s.%s" % (case, name)], float(golden["%s.err32.%s" % (case, name)])
        err = float(np.abs(value.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max())
        print("%s %-18s %.2e of the maximum, the reference's float32 run %.2e" % (case, name, err, err32))
        if not err <= max(4 * err32, 2.0 ** -23):
            worst.append((name, err, err32))
    assert not worst, worst


def test_training_mode_at_256_channels_draws_upstreams_masks_and_drops_the_same_rows(dev, bound):
    n, C, Hd, seed = 150, 256, 1024, 1234
    g = torch.Generator().manual_seed(77)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    params = {"norm.weight": 1 + 0.5 * r(C), "norm.bias": 0.1 * r(C), "fc1.weight": r(Hd, C) / C ** 0.5, "fc1.bias": 0.1 * r(Hd),
              "fc2.weight": r(C, Hd) / Hd ** 0.5, "fc2.bias": 0.1 * r(C)}
    feat, w = r(n, C) / 4, r(n, C)

    def run(forward, device, dtype, masks=None):
        block = _block(params, device, dtype, drop_path=0.3).train()
        drop = block.drop_path[0]
        if masks is not None:   # the float64 target replays the masks the GPU drew
            replay = iter(masks)
            drop.forward = lambda t: t * next(replay).to(device=t.device, dtype=t.dtype)
        x = feat.to(device=device, dtype=dtype).requires_grad_(True)
        torch.manual_seed(seed)
        point = forward(block, _point(x))
        (point.feat * w.to(device=device, dtype=dtype)).sum().backward()
        res = {"out": point.feat.detach().cpu(), "grad.feat": x.grad.cpu()}
        res.update({"grad." + k: p.grad.cpu() for k, p in block.named().items()})
        return res, [m.cpu() for m in drop.masks], point

    yard, masks, _ = run(upstream_forward, dev, torch.float32)
    assert len(masks) == 2 and bound.stats()["fused_calls"] == 0
    got, first, point = run(lambda b, p: b(p), dev, torch.float32)      # the rebound method
    assert bound.stats() == {"fused_calls": 1, "original_calls": 0} and bound.split_stats() == {"fused_calls": 1}
    assert len(first) == 1 and torch.equal(first[0], masks[0])            # the attention branch's mask, drawn first
    assert point.sparse_conv_feat.features is point.feat
    want, _, _ = run(upstream_forward, "cpu", torch.float64, masks)

    # the tail's shortcut: feat, doubled, then plus the first mask times itself -- the same bits on every path
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
