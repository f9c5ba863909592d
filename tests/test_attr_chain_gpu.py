"""-m gpu: the attribute head at inference in one launch per key (gaussiancity_amd.attr_chain -> modlinear.head_chain ->
gcm_head_chain, include/gcm.h).

  * against the REFERENCE's own results (tests/golden/attr_chain.npz, written by tests/golden/make_attr_chain_golden.py: the
    reference's GaussianAttrMLP under no_grad in float64, and the error of its own float32 run per tensor), without style
    codes and with them.  Bar, as test_attr_head_gpu: every output within 4 x the fixture's err32 of that tensor, as a
    fraction of the tensor's maximum -- the reference's own float32 run is that far from float64 under another summation
    order, and the 4 x absorbs the order.
  * the operator against its formula in torch float64 on the device; the bar is 4 x the error of the same formula in torch
    float32, measured here from torch (both as the largest difference over the tensor's largest float64 magnitude): the
    project's margin for another summation order.
  * a row's bits do not depend on the tile it falls into, on the row stride or on the run.
  * what the chain turns away returns, bit for bit, what the same module returns without the chain, and is counted.
  * the chained forward does not wait for the device.

The modules here are stand-ins written for the test: they hold parameters under upstream's names, and their own forward
raises unless a test asks for one that computes (the calls that both bindings turn away need a method to land on)."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attr_chain.npz")
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


def _stand_in(computes=False):
    """What install() needs of models/generator.py, written for this test.  computes: the head's own forward runs the zs
    None branch in torch ops (upstream's order of operations) instead of raising."""
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
        def __init__(self, z_dim, n_shared_layers, factors, n_layers, hidden=HIDDEN):
            super().__init__()
            self.factors, self.n_layers, self.n_shared_layers = factors, n_layers, n_shared_layers
            self.act = torch.nn.LeakyReLU(negative_slope=0.2)
            self.fc_m_a = torch.nn.Linear(CLASSES, hidden, bias=False)
            self.fc_1 = torch.nn.Linear(IN_DIM, hidden)
            layer = (lambda: torch.nn.Linear(hidden, hidden)) if z_dim is None else (lambda: ModLinear(hidden, hidden, z_dim))
            for i in range(2, n_shared_layers + 1):
                setattr(self, "fc_%d" % i, layer())
            for k in factors:
                for i in range(n_layers[k]):
                    setattr(self, "fc_%d_%s_%d" % (n_shared_layers + 1, k, i), layer())
                setattr(self, "fc_out_%s" % k, torch.nn.Linear(hidden, 1 if k == "opacity" else 3))

        def forward(self, pt_feat, onehots, zs):
            if not computes or zs is not None:
                raise AssertionError("the module's own GaussianAttrMLP.forward ran")
            f = self.act(self.fc_1(pt_feat) + self.fc_m_a(onehots))
            out = {}
            for k, factor in self.factors.items():
                h = f
                for i in range(self.n_layers[k]):
                    h = self.act(getattr(self, "fc_2_%s_%d" % (k, i))(f))
                v = getattr(self, "fc_out_%s" % k)(h)
                out[k] = torch.sigmoid(v) * factor + (1 - factor) if k == "opacity" else (torch.sigmoid(v) - 0.5) * factor
            return out

    return types.SimpleNamespace(GaussianAttrMLP=GaussianAttrMLP, ModLinear=ModLinear)


@pytest.fixture(scope="module")
def bound(dev):
    """A stand-in generator with attr_head and, over it, attr_chain installed, and the fixture."""
    from gaussiancity_amd import attr_chain, attr_head
    G = _stand_in()
    attr_head.install(G)
    attr_chain.install(G)
    yield G, np.load(GOLDEN)
    attr_chain.uninstall(G)
    attr_head.uninstall(G)


def _head(dev, G, gold, case):
    layers = {k: int(v) for k, v in zip(KEYS, gold[case + ".layers"]) if v >= 0}
    factors = {k: float(v) for k, v in zip(KEYS, gold[case + ".factors"]) if k in layers}
    z_dim = int(gold[case + ".z_dim"])
    head = G.GaussianAttrMLP(None if z_dim < 0 else z_dim, 1, factors, layers).to(dev)
    names = [n for n, _ in head.named_parameters()]
    assert sorted(names) == sorted(k[len(case) + 7:] for k in gold.files if k.startswith(case + ".param."))
    with torch.no_grad():
        for name in names:
            head.get_parameter(name).copy_(torch.from_numpy(gold["%s.param.%s" % (case, name)]))
    zs = ids = None
    if z_dim >= 0:
        ids = torch.from_numpy(gold[case + ".ids"]).to(dev)
        codes = torch.from_numpy(gold[case + ".z"]).to(dev)
        zs = {100 + g: {"z": codes[g:g + 1], "idx": (ids == g).unsqueeze(0)} for g in range(codes.shape[0])}
    feat = torch.from_numpy(gold[case + ".pt_feat"]).to(dev)
    onehots = torch.from_numpy(gold[case + ".onehots"]).to(dev)
    return head, factors, feat, onehots, zs, ids


@pytest.mark.parametrize("case", ["bg", "bg2", "bldg"])
def test_chained_head_matches_the_reference_in_float32(dev, bound, case):
    from gaussiancity_amd import attr_chain, modlinear
    G, gold = bound
    head, factors, feat, onehots, zs, ids = _head(dev, G, gold, case)
    attr_chain.reset_stats()
    modlinear.reset_stats()
    with torch.no_grad():
        out = head(feat, onehots, zs)
    assert attr_chain.stats() == {"chain_calls": 1, "passed_on_calls": 0}
    assert modlinear.chain_stats() == {"head_chain_calls": len(factors)} and modlinear.stats()["head_out_calls"] == 0
    assert list(out) == list(factors)
    worst = []
    for k, v in out.items():
        assert v.dtype == torch.float32 and v.device == feat.device
        assert tuple(v.shape) == (feat.shape[0], feat.shape[1], 1 if k == "opacity" else 3)
        if ids is not None:
            assert int((ids < 0).sum()) == 5 and not v[0][ids < 0].any(), k   # rows without a style: exact zeros
        want, err32 = gold["%s.out.%s" % (case, k)], float(gold["%s.err32.out.%s" % (case, k)])
        err = float(np.abs(v.double().cpu().numpy() - want).max() / np.abs(want).max())
        print("%s out.%-8s %.2e of the maximum, the reference's float32 run %.2e" % (case, k, err, err32))
        if not err <= 4 * err32:
            worst.append((k, err, err32))
    assert not worst, worst


# ---- the operator against its formula ------------------------------------------------------------------------------------
def _formula(dtype, t, kind, factor, slope):
    """head_chain's formula in torch ops of `dtype`; rows of group -1 are zeros."""
    c = {k: (v.to(dtype) if v is not None and v.is_floating_point() else v) for k, v in t.items()}
    act = lambda v: torch.nn.functional.leaky_relu(v, slope)  # noqa: E731
    f = act(c["x"] @ c["w1"].t() + c["onehots"] @ c["w_ma"].t() + c["b1"])
    g = None if c["group"] is None else c["group"].clamp(min=0).long()
    if c["alpha"] is not None:
        f = f * (c["alpha"][g] if g is not None else c["alpha"][0])
    h = f @ c["w2"].t()
    if c["beta"] is not None:
        h = h + (c["beta"][g] if g is not None else c["beta"][0])
    if c["bias2"] is not None:
        h = h + c["bias2"]
    v = act(h) @ c["w_out"].t() + c["b_out"]
    if kind == "scale":
        v = 1 + v.clamp(-1, 1) * factor
    elif kind == "opacity":
        v = torch.sigmoid(v) * factor + (1 - factor)
    else:
        v = (torch.sigmoid(v) - 0.5) * factor
    if c["group"] is not None:
        v = torch.where((c["group"] >= 0).unsqueeze(1), v, torch.zeros((), dtype=dtype, device=v.device))
    return v


def _operands(dev, N, I, K, H, G, C, seed):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(dev)  # noqa: E731
    t = {"x": rnd(N, I), "onehots": rnd(N, K), "w1": rnd(H, I, scale=I ** -0.5), "b1": rnd(H, scale=0.3),
         "w_ma": rnd(H, K, scale=0.5), "w2": rnd(H, H, scale=H ** -0.5), "alpha": None, "beta": None, "bias2": rnd(H, scale=0.3),
         "group": None, "w_out": rnd(C, H, scale=2.0 * H ** -0.5), "b_out": rnd(C, scale=0.3)}
    if G:
        t["alpha"], t["beta"], t["bias2"] = 1.0 + rnd(G, H, scale=0.5), rnd(G, H, scale=0.3), None
        group = torch.randint(0, G, (N,), generator=gen)
        group[torch.randperm(N, generator=gen)[:max(1, N // 9)]] = -1
        t["group"] = group.to(torch.int32).to(dev)
    return t


def _chain(t, kind, factor=0.75, slope=0.2):
    from gaussiancity_amd import modlinear
    return modlinear.head_chain(t["x"], t["onehots"], t["w1"], t["b1"], t["w_ma"], t["w2"], t["alpha"], t["beta"], t["bias2"],
                                t["group"], t["w_out"], t["b_out"], kind, factor, slope)


SHAPES = {  # N, I, K, H, G (0: no groups, a plain Linear with its bias)
    "one-row": (1, 4, 1, 4, 0),
    "fixture-sized": (63, 24, 7, 48, 0),
    "groups-80": (65, 124, 8, 80, 3),
    "full-lds": (130, 192, 8, 512, 0),
    "groups-512": (130, 124, 8, 512, 5),
}
OPERATOR_CASES = [(s, "rgb") for s in SHAPES if s != "groups-80"] + [("groups-80", k) for k in KEYS]


@pytest.mark.parametrize("shape,kind", OPERATOR_CASES, ids=["%s-%s" % c for c in OPERATOR_CASES])
def test_operator_against_its_formula_in_float64_on_the_device(dev, shape, kind):
    N, I, K, H, G = SHAPES[shape]
    t = _operands(dev, N, I, K, H, G, 1 if kind == "opacity" else 3, seed=sorted(SHAPES).index(shape))
    factor = 0.5 if kind == "scale" else 0.75
    with torch.no_grad():
        want, own32 = _formula(torch.float64, t, kind, factor, 0.2), _formula(torch.float32, t, kind, factor, 0.2)
        got = _chain(t, kind, factor)
    assert got.dtype == torch.float32 and got.shape == want.shape
    top = float(want.abs().max())
    bar, err = 4 * float((own32.double() - want).abs().max()) / top, float((got.double() - want).abs().max()) / top
    print("%s %s: %.2e of the maximum, bar %.2e (4 x torch float32)" % (shape, kind, err, bar))
    if G:
        assert (t["group"] < 0).any() and not got[t["group"] < 0].any()
    if kind == "scale":
        clamped = (want[t["group"] >= 0] - 1).abs() >= factor - 1e-12
        assert clamped.any() and not clamped.all()
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("shape", ["full-lds", "groups-512"])
def test_a_rows_bits_do_not_depend_on_the_tile_the_stride_or_the_run(dev, shape):
    N, I, K, H, G = SHAPES[shape]
    t = _operands(dev, N, I, K, H, G, 3, seed=7)
    with torch.no_grad():
        whole = _chain(t, "rgb")
        assert torch.equal(whole, _chain(t, "rgb"))
        for a, b in ((0, 1), (63, 65), (64, 130)):
            part = dict(t, x=t["x"][a:b], onehots=t["onehots"][a:b], group=None if t["group"] is None else t["group"][a:b])
            assert torch.equal(whole[a:b], _chain(part, "rgb")), (a, b)
        wide = torch.randn(N, I + 12, device=dev)
        wide[:, 4:4 + I] = t["x"]
        sliced = wide[:, 4:4 + I]
        assert sliced.stride(0) == I + 12 and not sliced.is_contiguous()
        hot = torch.randn(N, K + 3, device=dev)
        hot[:, 1:1 + K] = t["onehots"]
        assert torch.equal(whole, _chain(dict(t, x=sliced, onehots=hot[:, 1:1 + K]), "rgb"))
        empty = _chain(dict(t, x=t["x"][:0], onehots=t["onehots"][:0], group=None if t["group"] is None else t["group"][:0]), "rgb")
    assert tuple(empty.shape) == (0, 3) and empty.dtype == torch.float32 and empty.device == whole.device


# ---- what the chain turns away -------------------------------------------------------------------------------------------
def _random_head(dev, G, z_dim, n_shared, factors, layers, hidden=HIDDEN, seed=5):
    head = G.GaussianAttrMLP(z_dim, n_shared, factors, layers, hidden)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in head.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.3 if p.dim() == 1 else p.shape[1] ** -0.5))
            if name.endswith("bias_alpha"):
                p.add_(1.0)
    return head.to(dev)


def _inputs(dev, n=70, instances=3, seed=9):
    gen = torch.Generator().manual_seed(seed)
    feat = torch.randn(1, n, IN_DIM, generator=gen).to(dev)
    onehots = torch.eye(CLASSES)[torch.randint(0, CLASSES, (n,), generator=gen)].unsqueeze(0).to(dev)
    ids = torch.randint(-1, instances, (n,), generator=gen).to(dev)
    codes = torch.randn(instances, Z_DIM, generator=gen).to(dev)
    zs = {100 + g: {"z": codes[g:g + 1], "idx": (ids == g).unsqueeze(0)} for g in range(instances)}
    return feat, onehots, zs


TURNED_AWAY = ["gradients", "H=516", "two shared layers", "two layers under codes", "autocast", "float16"]


@pytest.mark.parametrize("what", TURNED_AWAY)
def test_what_is_turned_away_keeps_its_bits_and_is_counted(dev, what):
    from gaussiancity_amd import attr_chain, attr_head
    G = _stand_in(computes=True)
    factors, one = {"rgb": 2.0, "opacity": 0.6}, {"rgb": 1, "opacity": 1}
    feat, onehots, zs = _inputs(dev)
    if what == "gradients":
        head = _random_head(dev, G, Z_DIM, 1, factors, one)
    elif what == "H=516":
        head = _random_head(dev, G, Z_DIM, 1, factors, one, hidden=516)
    elif what == "two shared layers":
        head = _random_head(dev, G, Z_DIM, 2, factors, one)
    elif what == "two layers under codes":
        head = _random_head(dev, G, Z_DIM, 1, factors, {"rgb": 2, "opacity": 1})
    else:  # nothing of either binding runs these: the module's own method does
        head, zs = _random_head(dev, G, None, 1, factors, one), None
        if what == "float16":
            head, feat, onehots = head.half(), feat.half(), onehots.half()

    def call():
        attr_head.reset_stats()
        with torch.set_grad_enabled(what == "gradients"), torch.autocast("cuda", dtype=torch.float16, enabled=what == "autocast"):
            out = head(feat, onehots, zs)
        return {k: v.detach() for k, v in out.items()}, attr_head.stats()

    attr_head.install(G)
    attr_chain.install(G)
    try:
        attr_chain.reset_stats()
        with_chain, counted_with = call()
        assert attr_chain.stats() == {"chain_calls": 0, "passed_on_calls": 1}
        attr_chain.uninstall(G)
        without, counted_without = call()
        assert attr_chain.stats() == {"chain_calls": 0, "passed_on_calls": 1}
    finally:
        attr_chain.uninstall(G)
        attr_head.uninstall(G)
    assert counted_with == counted_without == ({"fused_calls": 0, "original_calls": 1} if zs is None else
                                               {"fused_calls": 1, "original_calls": 0})
    assert list(with_chain) == list(without) == list(factors)
    for k in factors:
        assert with_chain[k].dtype == without[k].dtype and torch.equal(with_chain[k], without[k]), k
        assert bool(torch.isfinite(with_chain[k]).all()) and bool(with_chain[k].any())


def test_chained_forward_does_not_wait_for_the_device(dev, bound):
    """The chained no_grad forward, with style codes, under torch.cuda.set_sync_debug_mode("error"): any host wait raises."""
    from gaussiancity_amd import attr_chain
    G, gold = bound
    head, _, feat, onehots, zs, _ = _head(dev, G, gold, "bldg")
    with torch.no_grad():
        head(feat, onehots, zs)   # first call outside the mode: the library loads, kernels' code objects load
        torch.cuda.synchronize()
        attr_chain.reset_stats()
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
    assert attr_chain.stats() == {"chain_calls": 1, "passed_on_calls": 0}
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
