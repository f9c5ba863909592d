"""-m gpu: the binding of the generator's attribute head (gaussiancity_amd.attr_head -> modlinear -> include/gcm.h)
against the REFERENCE's own results (tests/golden/attr_head.npz, written by tests/golden/make_attr_head_golden.py: the
reference's GaussianAttrMLP with a `zs` dict in float64, and the error of its own float32 run per tensor).

The modules here are stand-ins written for the test: they hold parameters under upstream's names and their own forward
raises, so whatever the test computes comes from the rebound method.  Bar, as
test_backbone_binding_matches_the_reference_in_float32: every output and every gradient within 4 x the fixture's err32
of that tensor, as a fraction of the tensor's maximum -- the reference's own float32 run is that far from float64 under
another summation order, and the 4 x absorbs the order."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attr_head.npz")
KEYS = ("xyz", "rgb", "scale", "opacity")
HIDDEN, Z_DIM, IN_DIM, CLASSES = 48, 16, 24, 7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _stand_in():
    """What install() needs of models/generator.py, written for this test.  Every forward of its own raises."""
    class ModLinear(torch.nn.Module):
        def __init__(self, in_features, out_features, style_features):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.zeros(out_features, in_features))
            self.bias, self.mod_bias, self.output_mode = None, True, True
            self.weight_alpha = torch.nn.Parameter(torch.zeros(in_features, style_features))
            self.bias_alpha = torch.nn.Parameter(torch.zeros(in_features))
            self.weight_beta = torch.nn.Parameter(torch.zeros(out_features, style_features))
            self.bias_beta = torch.nn.Parameter(torch.zeros(out_features))

        def forward(self, x, z):
            raise AssertionError("the module's own ModLinear.forward ran")

    class GaussianAttrMLP(torch.nn.Module):
        def __init__(self, n_shared_layers, factors, n_layers):
            super().__init__()
            self.factors, self.n_layers, self.n_shared_layers = factors, n_layers, n_shared_layers
            self.act = torch.nn.LeakyReLU(negative_slope=0.2)
            self.fc_m_a = torch.nn.Linear(CLASSES, HIDDEN, bias=False)
            self.fc_1 = torch.nn.Linear(IN_DIM, HIDDEN)
            for i in range(2, n_shared_layers + 1):
                setattr(self, "fc_%d" % i, ModLinear(HIDDEN, HIDDEN, Z_DIM))
            for k in factors:
                for i in range(n_layers[k]):
                    setattr(self, "fc_%d_%s_%d" % (n_shared_layers + 1, k, i), ModLinear(HIDDEN, HIDDEN, Z_DIM))
                setattr(self, "fc_out_%s" % k, torch.nn.Linear(HIDDEN, 1 if k == "opacity" else 3))

        def forward(self, pt_feat, onehots, zs):
            raise AssertionError("the module's own GaussianAttrMLP.forward ran")

    return types.SimpleNamespace(GaussianAttrMLP=GaussianAttrMLP, ModLinear=ModLinear)


@pytest.fixture(scope="module")
def bound(dev):
    from gaussiancity_amd import attr_head
    G = _stand_in()
    attr_head.install(G)
    yield G, np.load(GOLDEN)
    attr_head.uninstall(G)


def _head(dev, G, gold, case):
    layers = {k: int(v) for k, v in zip(KEYS, gold[case + ".layers"]) if v >= 0}
    factors = {k: float(v) for k, v in zip(KEYS, gold[case + ".factors"]) if k in layers}
    head = G.GaussianAttrMLP(int(gold[case + ".n_shared"]), factors, layers).to(dev)
    names = [n for n, _ in head.named_parameters()]
    assert sorted(names) == sorted(k[len(case) + 7:] for k in gold.files if k.startswith(case + ".param."))
    with torch.no_grad():
        for name in names:
            head.get_parameter(name).copy_(torch.from_numpy(gold["%s.param.%s" % (case, name)]))
    ids = torch.from_numpy(gold[case + ".ids"]).to(dev)
    codes = torch.from_numpy(gold[case + ".z"]).to(dev)
    zs = {100 + g: {"z": codes[g:g + 1], "idx": (ids == g).unsqueeze(0)} for g in range(codes.shape[0])}
    feat = torch.from_numpy(gold[case + ".pt_feat"]).to(dev)
    onehots = torch.from_numpy(gold[case + ".onehots"]).to(dev)
    return head, names, factors, feat, onehots, zs, ids


def _hold(gold, case, got):
    worst = []
    for name, value in got.items():
        want, err32 = gold["%s.%s" % (case, name)], float(gold["%s.err32.%s" % (case, name)])
        assert value.shape == want.shape, (name, value.shape, want.shape)
        err = float(np.abs(value - want).max() / np.abs(want).max())
        print("%s %-32s %.2e of the maximum, the reference's float32 run %.2e" % (case, name, err, err32))
        if not err <= 4 * err32:
            worst.append((name, err, err32))
    assert not worst, worst


@pytest.mark.parametrize("case", ["a", "b"])
def test_head_binding_matches_the_reference_in_float32(dev, bound, case):
    from gaussiancity_amd import attr_head
    G, gold = bound
    head, names, factors, feat, onehots, zs, ids = _head(dev, G, gold, case)
    feat.requires_grad_(True)
    attr_head.reset_stats()
    out = head(feat, onehots, zs)
    assert attr_head.stats() == {"fused_calls": 1, "original_calls": 0}
    assert list(out) == list(factors)
    for k, v in out.items():
        assert v.dtype == torch.float32 and v.device == feat.device
        assert tuple(v.shape) == (1, feat.shape[1], 1 if k == "opacity" else 3)
        assert not v[0][ids < 0].any(), k   # rows without a style: exact zeros
    sum((out[k] * torch.from_numpy(gold["%s.w.%s" % (case, k)]).to(dev)).sum() for k in factors).backward()
    got = {"out." + k: v.detach() for k, v in out.items()}
    got["grad.pt_feat"] = feat.grad
    got.update({"grad." + name: head.get_parameter(name).grad for name in names})
    _hold(gold, case, {k: v.double().cpu().numpy() for k, v in got.items()})


@pytest.mark.parametrize("case", ["a", "b"])
def test_inference_path_through_head_out_matches_the_reference(dev, bound, case):
    from gaussiancity_amd import attr_head, modlinear
    G, gold = bound
    head, _, factors, feat, onehots, zs, ids = _head(dev, G, gold, case)
    attr_head.reset_stats()
    modlinear.reset_stats()
    with torch.no_grad():
        out = head(feat, onehots, zs)
    assert attr_head.stats() == {"fused_calls": 1, "original_calls": 0}
    assert modlinear.stats()["head_out_calls"] == len(factors) and modlinear.stats()["groups_from_masks_calls"] == 1
    for k, v in out.items():
        assert v.dtype == torch.float32 and tuple(v.shape) == (1, feat.shape[1], 1 if k == "opacity" else 3)
        assert not v[0][ids < 0].any(), k
    _hold(gold, case, {"out." + k: v.double().cpu().numpy() for k, v in out.items()})


def test_inference_forward_does_not_wait_for_the_device(dev, bound):
    """The fused no_grad forward under torch.cuda.set_sync_debug_mode("error"): any host wait raises."""
    G, gold = bound
    head, _, _, feat, onehots, zs, _ = _head(dev, G, gold, "a")
    with torch.no_grad():
        head(feat, onehots, zs)   # first call outside the mode: the library loads, kernels' code objects load
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            try:
                feat.sum().item()
                flagged = False
            except RuntimeError:
                flagged = True
            if flagged:
                out = head(feat, onehots, zs)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    if not flagged:
        pytest.skip("this torch build does not flag .item() under set_sync_debug_mode('error')")
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
