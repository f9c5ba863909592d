"""-m gpu: attr_head.install(generator, fused_outputs=True) and attr_head.gaussian_points (-> modlinear.head_attrs /
head_points14 -> gcm_head_train_*) against the REFERENCE's own results: tests/golden/attr_head.npz
(style codes) and tests/golden/attr_head_plain.npz (z_dim=None and zs None, written by
tests/golden/make_attr_head_plain_golden.py).

The modules are stand-ins as in tests/test_attr_head_gpu.py: parameters under upstream's names, and a forward of their own
that raises, so whatever the test computes comes from the rebound method (a plain Linear is torch's and does run: the
binding calls the module's own layers for zs None).  The bar is that file's: every output and gradient within 4 x the
fixture's err32 of that tensor, as a fraction of the tensor's maximum."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xyz", "rgb", "scale", "opacity")
AT = {"xyz": (0, 3), "opacity": (3, 4), "scale": (4, 7), "rgb": (11, 14)}
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


@pytest.fixture(scope="module")
def golds():
    return {"codes": np.load(os.path.join(HERE, "golden", "attr_head.npz")),
            "plain": np.load(os.path.join(HERE, "golden", "attr_head_plain.npz"))}


def _stand_in():
    """What install() needs of models/generator.py, written for this test.  plain: the layers z_dim=None builds."""
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
        def __init__(self, n_shared_layers, factors, n_layers, plain):
            super().__init__()
            self.factors, self.n_layers, self.n_shared_layers = factors, n_layers, n_shared_layers
            self.act = torch.nn.LeakyReLU(negative_slope=0.2)
            self.fc_m_a = torch.nn.Linear(CLASSES, HIDDEN, bias=False)
            self.fc_1 = torch.nn.Linear(IN_DIM, HIDDEN)
            layer = (lambda: torch.nn.Linear(HIDDEN, HIDDEN)) if plain else (lambda: ModLinear(HIDDEN, HIDDEN, Z_DIM))
            for i in range(2, n_shared_layers + 1):
                setattr(self, "fc_%d" % i, layer())
            for k in factors:
                for i in range(n_layers[k]):
                    setattr(self, "fc_%d_%s_%d" % (n_shared_layers + 1, k, i), layer())
                setattr(self, "fc_out_%s" % k, torch.nn.Linear(HIDDEN, 1 if k == "opacity" else 3))

        def forward(self, pt_feat, onehots, zs):
            raise AssertionError("the module's own GaussianAttrMLP.forward ran")

    return types.SimpleNamespace(GaussianAttrMLP=GaussianAttrMLP, ModLinear=ModLinear)


@pytest.fixture()
def fused(dev):
    from gaussiancity_amd import attr_head
    G = _stand_in()
    attr_head.install(G, fused_outputs=True)
    yield G
    attr_head.uninstall(G)


def _head(dev, G, gold, case, plain):
    layers = {k: int(v) for k, v in zip(KEYS, gold[case + ".layers"]) if v >= 0}
    factors = {k: float(v) for k, v in zip(KEYS, gold[case + ".factors"]) if k in layers}
    if plain:   # the fixture's key order is the reference's dict order
        order = [k[len(case) + 5:] for k in gold.files if k.startswith(case + ".out.")]
        layers, factors = {k: layers[k] for k in order}, {k: factors[k] for k in order}
    head = G.GaussianAttrMLP(int(gold[case + ".n_shared"]), factors, layers, plain).to(dev)
    names = [n for n, _ in head.named_parameters()]
    assert sorted(names) == sorted(k[len(case) + 7:] for k in gold.files if k.startswith(case + ".param."))
    with torch.no_grad():
        for name in names:
            head.get_parameter(name).copy_(torch.from_numpy(gold["%s.param.%s" % (case, name)]))
    feat = torch.from_numpy(gold[case + ".pt_feat"]).to(dev).requires_grad_(True)
    onehots = torch.from_numpy(gold[case + ".onehots"]).to(dev)
    zs, ids = None, None
    if not plain:
        ids = torch.from_numpy(gold[case + ".ids"]).to(dev)
        codes = torch.from_numpy(gold[case + ".z"]).to(dev)
        zs = {100 + g: {"z": codes[g:g + 1], "idx": (ids == g).unsqueeze(0)} for g in range(codes.shape[0])}
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


def _grads(gold, case, head, names, feat):
    """The gradients the fixture holds; a parameter the reference does not use has none here either."""
    got = {"grad.pt_feat": feat.grad}
    for name in names:
        grad = head.get_parameter(name).grad
        if "%s.grad.%s" % (case, name) in gold.files:
            got["grad." + name] = grad
        else:
            assert grad is None, name
    return got


@pytest.mark.parametrize("kind,case", [("codes", "a"), ("codes", "b"), ("plain", "a"), ("plain", "b")])
def test_fused_outputs_match_the_reference_in_float32(dev, fused, golds, kind, case):
    from gaussiancity_amd import attr_head, modlinear
    gold, plain = golds[kind], kind == "plain"
    head, names, factors, feat, onehots, zs, ids = _head(dev, fused, gold, case, plain)
    attr_head.reset_stats()
    modlinear.reset_stats()
    out = head(feat, onehots, zs)
    assert attr_head.stats() == {"fused_calls": 1, "original_calls": 0}
    assert attr_head.output_stats() == {"head_attrs_calls": 1, "head_points14_calls": 0}
    assert list(out) == list(factors)
    for k, v in out.items():
        assert v.dtype == torch.float32 and v.device == feat.device
        assert tuple(v.shape) == (1, feat.shape[1], 1 if k == "opacity" else 3)
        if ids is not None:
            assert not v[0][ids < 0].any(), k   # rows without a style: exact zeros
    sum((out[k] * torch.from_numpy(gold["%s.w.%s" % (case, k)]).to(dev)).sum() for k in factors).backward()
    s = modlinear.head_train_stats()
    assert s["forward_calls"] == 1 and s["backward_calls"] == 1 and s["dh_outputs"] == len(factors)
    assert modlinear.stats()["head_out_calls"] == 0
    got = {"out." + k: v.detach() for k, v in out.items()}
    got.update(_grads(gold, case, head, names, feat))
    _hold(gold, case, {k: v.double().cpu().numpy() for k, v in got.items()})


@pytest.mark.parametrize("kind,case", [("codes", "a"), ("codes", "b"), ("plain", "a"), ("plain", "b")])
def test_gaussian_points_matches_get_gaussian_points_of_the_reference(dev, fused, golds, kind, case):
    """The [1, N, 14] record against helpers.get_gaussian_points of the golden float64 attributes, per attribute's columns
    within 4 x that attribute's err32; the loss weights every attribute's columns so that the gradients are the fixture's:
    d(xyz + a)/da = 1, d(scales * a)/da = scales.  xyz is kept small against the offsets (0.05 sigma against up to 0.37):
    the record stores xyz + a in float32, and half a unit of a large xyz would be an error of the FORMAT, several err32 of
    the attribute, on both this side and the reference's; the scale columns are divided by scales before they are compared."""
    from gaussiancity_amd import attr_head, helpers, modlinear
    gold, plain = golds[kind], kind == "plain"
    head, names, factors, feat, onehots, zs, _ = _head(dev, fused, gold, case, plain)
    n = feat.shape[1]
    rng = np.random.default_rng(5)
    xyz = torch.from_numpy((0.05 * rng.normal(size=(1, n, 3))).astype(np.float32)).to(dev)
    scales = torch.from_numpy(rng.uniform(0.5, 2.0, size=(1, n, 3)).astype(np.float32)).to(dev)
    keep = xyz.clone(), scales.clone()
    attr_head.reset_stats()
    modlinear.reset_stats()
    points = attr_head.gaussian_points(head, feat, onehots, zs, xyz, scales)
    assert tuple(points.shape) == (1, n, 14) and points.dtype == torch.float32
    assert torch.equal(xyz, keep[0]) and torch.equal(scales, keep[1])
    assert attr_head.output_stats() == {"head_attrs_calls": 0, "head_points14_calls": 1}
    want = helpers.get_gaussian_points(xyz.double().cpu(), scales.double().cpu(),
                                       {k: torch.from_numpy(gold["%s.out.%s" % (case, k)]) for k in factors})[0].numpy()
    got = points[0].detach().double().cpu().numpy()
    assert got[:, 7:11].tobytes() == want[:, 7:11].tobytes()
    worst = []
    for k, (a, b) in AT.items():
        if k not in factors:
            assert got[:, a:b].tobytes() == want[:, a:b].tobytes(), k
            continue
        attr64 = gold["%s.out.%s" % (case, k)][0]
        gain = scales[0].double().cpu().numpy() if k == "scale" else 1.0   # the record's error is the attribute's times this
        err = float((np.abs(got[:, a:b] - want[:, a:b]) / gain).max() / np.abs(attr64).max())
        err32 = float(gold["%s.err32.out.%s" % (case, k)])
        print("%s %-8s %.2e of the maximum, the reference's float32 run %.2e" % (case, k, err, err32))
        if not err <= 4 * err32:
            worst.append((k, err, err32))
    assert not worst, worst
    weight = torch.zeros(1, n, 14, device=dev)
    for k in factors:
        w = torch.from_numpy(gold["%s.w.%s" % (case, k)]).to(dev)
        weight[..., AT[k][0]:AT[k][1]] = w / scales if k == "scale" else w
    (points * weight).sum().backward()
    assert modlinear.head_train_stats()["backward_calls"] == 1
    _hold(gold, case, {k: v.double().cpu().numpy() for k, v in _grads(gold, case, head, names, feat).items()})


def test_the_default_install_does_not_reach_the_new_operator(dev, golds):
    from gaussiancity_amd import attr_head, modlinear
    G = _stand_in()
    before = G.GaussianAttrMLP.forward
    attr_head.install(G)
    try:
        head, _, factors, feat, onehots, zs, _ = _head(dev, G, golds["codes"], "a", False)
        attr_head.reset_stats()
        modlinear.reset_stats()
        out = head(feat, onehots, zs)
        sum(v.sum() for v in out.values()).backward()
        assert attr_head.stats() == {"fused_calls": 1, "original_calls": 0}
        assert not any(modlinear.head_train_stats().values()) and not any(attr_head.output_stats().values())
        plain, _, _, pfeat, ponehots, _, _ = _head(dev, G, golds["plain"], "a", True)
        with pytest.raises(AssertionError, match="own GaussianAttrMLP.forward ran"):
            plain(pfeat, ponehots, None)   # zs None goes to the module's own method, as before
        assert attr_head.stats() == {"fused_calls": 1, "original_calls": 1}
    finally:
        attr_head.uninstall(G)
    assert G.GaussianAttrMLP.forward is before and not hasattr(G, attr_head._ORIGINAL)


def test_no_grad_calls_still_go_through_head_out(dev, fused, golds):
    from gaussiancity_amd import attr_head, modlinear
    gold = golds["codes"]
    head, _, factors, feat, onehots, zs, _ = _head(dev, fused, gold, "a", False)
    attr_head.reset_stats()
    modlinear.reset_stats()
    with torch.no_grad():
        out = head(feat, onehots, zs)
    assert attr_head.stats() == {"fused_calls": 1, "original_calls": 0}
    assert modlinear.stats()["head_out_calls"] == len(factors) and not any(modlinear.head_train_stats().values())
    assert not any(attr_head.output_stats().values())
    _hold(gold, "a", {"out." + k: v.double().cpu().numpy() for k, v in out.items()})
    plain, _, _, pfeat, ponehots, _, _ = _head(dev, fused, golds["plain"], "a", True)
    with torch.no_grad(), pytest.raises(AssertionError, match="own GaussianAttrMLP.forward ran"):
        plain(pfeat, ponehots, None)   # zs None without gradients: the module's own method


def test_fused_and_default_installs_agree_bit_for_bit_on_the_outputs(dev, golds):
    """head_attrs has head_out's bits; torch's tail is another summation, so the two installs are compared through the
    inference path of the default one."""
    from gaussiancity_amd import attr_head
    G = _stand_in()
    attr_head.install(G, fused_outputs=True)
    try:
        head, _, _, feat, onehots, zs, _ = _head(dev, G, golds["codes"], "a", False)
        with_grad = head(feat, onehots, zs)
        with torch.no_grad():
            without = head(feat, onehots, zs)
        for k in with_grad:
            assert torch.equal(with_grad[k].detach(), without[k]), k
    finally:
        attr_head.uninstall(G)
