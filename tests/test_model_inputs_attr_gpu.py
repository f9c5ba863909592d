"""-m gpu: the attribute head fed with the split's GroupedCodes (gaussiancity_amd.model_inputs) instead of _get_z's dict.
attr_head and attr_chain take its group vector and code table as they are -- no groups_from_masks, no torch.cat -- and must
return identical bits; the module's own method, which only knows `zs is None` and `zs.values()`, must not notice the
difference; torch.nn.DataParallel must hand the object through untouched.

The modules are stand-ins written for the test, as in test_attr_chain_gpu: parameters under upstream's names, and an own
forward that walks zs.values() the way upstream's does (one masked gather, one modulated stack and one masked store per
instance)."""
import types

import numpy as np
import pytest
import torch

import model_inputs_ref as R

pytestmark = pytest.mark.gpu
HIDDEN, Z_DIM, IN_DIM, CLASSES = 48, 16, 24, 8
FACTORS = {"xyz": 0.5, "rgb": 1.0, "scale": 0.3, "opacity": 0.8}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m, _native_v
    _native_m.lib()
    _native_v.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _stand_in():
    class ModLinear(torch.nn.Module):
        def __init__(self, in_features, out_features, style_features):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.randn(out_features, in_features) / in_features ** 0.5)
            self.bias, self.mod_bias, self.output_mode = None, True, True
            self.weight_alpha = torch.nn.Parameter(torch.randn(in_features, style_features) / style_features ** 0.5)
            self.bias_alpha = torch.nn.Parameter(torch.ones(in_features))
            self.weight_beta = torch.nn.Parameter(torch.randn(out_features, style_features) / style_features ** 0.5)
            self.bias_beta = torch.nn.Parameter(torch.zeros(out_features))

        def forward(self, x, z):   # modulate the input, multiply, add the modulated bias
            alpha = torch.addmm(self.bias_alpha, z, self.weight_alpha.t())
            beta = torch.addmm(self.bias_beta, z, self.weight_beta.t())
            return (x * alpha.unsqueeze(1)) @ self.weight.t() + beta.unsqueeze(1)

    class GaussianAttrMLP(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.factors, self.n_layers, self.n_shared_layers = dict(FACTORS), dict.fromkeys(FACTORS, 1), 1
            self.act = torch.nn.LeakyReLU(negative_slope=0.2)
            self.fc_m_a = torch.nn.Linear(CLASSES, HIDDEN, bias=False)
            self.fc_1 = torch.nn.Linear(IN_DIM, HIDDEN)
            for k in FACTORS:
                setattr(self, "fc_2_%s_0" % k, ModLinear(HIDDEN, HIDDEN, Z_DIM))
                setattr(self, "fc_out_%s" % k, torch.nn.Linear(HIDDEN, 1 if k == "opacity" else 3))

        def forward(self, pt_feat, onehots, zs):
            assert zs is not None
            b, n, _ = pt_feat.size()
            f = self.act(self.fc_1(pt_feat) + self.fc_m_a(onehots))
            output = {k: torch.zeros(b, n, 1 if k == "opacity" else 3, device=pt_feat.device) for k in self.factors}
            for v in zs.values():
                z, idx = v["z"], v["idx"]
                fi = f[idx].unsqueeze(0)
                for k, factor in self.factors.items():
                    h = self.act(getattr(self, "fc_2_%s_0" % k)(fi, z))
                    o = getattr(self, "fc_out_%s" % k)(h)
                    if k == "scale":
                        o = 1 + o.clamp(-1, 1) * factor
                    elif k == "opacity":
                        o = torch.sigmoid(o) * factor + (1 - factor)
                    else:
                        o = (torch.sigmoid(o) - 0.5) * factor
                    output[k][idx] = o
            return output

    return types.SimpleNamespace(GaussianAttrMLP=GaussianAttrMLP, ModLinear=ModLinear)


@pytest.fixture(scope="module")
def case(dev):
    """The building rows of a small frame through split_by_model: 5 buildings, 3 of them with a code (one without in the
    middle of the order), so some rows have group -1."""
    from gaussiancity_amd import model_inputs as MI
    from gaussiancity_amd import points as P
    rng = np.random.default_rng(1703)
    ids = np.array([1, 4, 100, 101, 340, 341, 2000, 10000], np.int16)
    m = 600
    ins = ids[rng.integers(0, len(ids), m)]
    ins[:len(ids)] = ids
    pts = np.zeros((m, 8), np.float32)
    pts[:, :3], pts[:, 4] = rng.integers(0, 2048, (m, 3)), ins
    cls = np.where(ins >= 10000, 3, np.where(ins >= 100, np.where(ins % 2 == 0, 2, 7), ins)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    vs = P.VisibleSet(torch.arange(m, device=dev), t(pts)[None], t(np.searchsorted(ids, ins).astype(np.int32)).reshape(1, m, 1),
                      t(ids), t(cls).reshape(1, m, 1), torch.ones((1, m, 3), device=dev))
    gen = torch.Generator().manual_seed(9)
    lut = {i: torch.randn(1, Z_DIM, generator=gen) for i in (100, 340, 2000, 4, 555)}
    split = MI.split_by_model(vs, MI.MODEL_RULE_KITTI_360(), lut)
    bldg = split.models["BLDG"]
    zs = bldg.zs
    assert isinstance(zs, MI.GroupedCodes) and list(zs) == [100, 340, 2000] and bool((zs.group == -1).any())
    as_dict = {i: {"z": v["z"].clone(), "idx": v["idx"].clone()} for i, v in zs.items()}     # what _get_z returns
    want = R.get_z(pts[np.isin(cls, (2, 7)), 4], {i: z[0].numpy() for i, z in lut.items()})
    assert list(as_dict) == list(want) and all(np.array_equal(as_dict[i]["idx"].cpu().numpy(), want[i]["idx"]) for i in want)
    n = bldg.index.shape[0]
    feat = torch.randn((1, n, IN_DIM), generator=torch.Generator().manual_seed(10)).to(dev)
    torch.manual_seed(11)
    G = _stand_in()
    head = G.GaussianAttrMLP().to(dev)
    return G, head, feat, bldg.onehots, zs, as_dict


def _bits_equal(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_own_method_cannot_tell_grouped_codes_from_the_dict(case):
    G, head, feat, onehots, zs, as_dict = case
    with torch.no_grad():
        _bits_equal(head(feat, onehots, zs), head(feat, onehots, as_dict))


def test_attr_head_takes_group_and_codes_as_they_are(case):
    from gaussiancity_amd import attr_head, modlinear
    G, head, feat, onehots, zs, as_dict = case
    attr_head.install(G)
    try:
        for grad in (True, False):
            with torch.set_grad_enabled(grad):
                attr_head.reset_stats()
                modlinear.reset_stats()
                from_dict = head(feat, onehots, as_dict)
                assert attr_head.stats() == {"fused_calls": 1, "original_calls": 0} and attr_head.grouped_stats() == {"grouped_calls": 0}
                assert modlinear.stats()["groups_from_masks_calls"] == 1
                grouped = head(feat, onehots, zs)
                assert attr_head.stats() == {"fused_calls": 2, "original_calls": 0} and attr_head.grouped_stats() == {"grouped_calls": 1}
                assert modlinear.stats()["groups_from_masks_calls"] == 1                  # no masks were folded
                _bits_equal({k: v.detach() for k, v in grouped.items()}, {k: v.detach() for k, v in from_dict.items()})
        with torch.no_grad():                               # and the fused result is the module's own, to float32 accuracy
            attr_head.uninstall(G)
            own = head(feat, onehots, zs)
            attr_head.install(G)
        for k in own:
            assert float((own[k] - grouped[k]).abs().max()) < 1e-4, k
    finally:
        attr_head.uninstall(G)


def test_attr_chain_takes_group_and_codes_as_they_are(case):
    from gaussiancity_amd import attr_chain, attr_head, modlinear
    G, head, feat, onehots, zs, as_dict = case
    attr_head.install(G)
    attr_chain.install(G)
    try:
        with torch.no_grad():
            attr_chain.reset_stats()
            modlinear.reset_stats()
            from_dict = head(feat, onehots, as_dict)
            assert attr_chain.stats() == {"chain_calls": 1, "passed_on_calls": 0} and attr_chain.grouped_stats() == {"grouped_calls": 0}
            grouped = head(feat, onehots, zs)
            assert attr_chain.stats() == {"chain_calls": 2, "passed_on_calls": 0} and attr_chain.grouped_stats() == {"grouped_calls": 1}
            assert modlinear.stats()["groups_from_masks_calls"] == 1 and modlinear.chain_stats() == {"head_chain_calls": 2 * len(FACTORS)}
            _bits_equal(grouped, from_dict)
    finally:
        attr_chain.uninstall(G)
        attr_head.uninstall(G)


def test_grouped_codes_survives_data_parallel_as_the_same_object(case, dev):
    G, head, feat, onehots, zs, as_dict = case
    seen = []

    class Probe(torch.nn.Module):
        def forward(self, x, zs):
            seen.append(zs)
            return x

    model = torch.nn.DataParallel(Probe(), device_ids=[0]).to(dev)
    model(feat, zs)
    model(feat, zs=as_dict)
    assert seen[0] is zs                      # scatter leaves what is not a tensor, tuple, list or dict alone
    assert seen[1] is not as_dict and list(seen[1]) == list(as_dict)    # (a dict is rebuilt)
