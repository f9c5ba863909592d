"""gcm_head_chain and gaussiancity_amd.attr_chain without a GPU (not gpu): every argument rule of the header comes back as
GCM_ERR_INVALID_ARGUMENT with a message, on host pointers that are never dereferenced, before a device is touched;
attr_chain.install / uninstall rebind and restore the method of a stand-in models.generator, alone and together with
attr_head in both orders; CPU tensors and calls with gradients enabled reach the method that was bound before and are
counted."""
import ctypes as C
import types

import pytest
import torch

from gaussiancity_amd import _native_m as M
from gaussiancity_amd import attr_chain, attr_head, modlinear

INVALID = -1  # GCM_ERR_INVALID_ARGUMENT


@pytest.fixture()
def mem():
    """(the library, a 256-byte aligned address of host memory that no call below reaches the point of using)."""
    buf = (C.c_float * 1024)()
    return M.lib(), buf, (C.addressof(buf) + 255) // 256 * 256


def _chain(lib, p, N=4, I=8, K=7, H=8, G=1, Cn=3, kind=1, factor=0.5, slope=0.2, xs=8, hs=7, w1s=8, w2s=8, **ptrs):
    a = {name: p for name in ("x", "onehots", "w1", "b1", "w_ma", "w2", "w_out", "out")}
    a.update({name: None for name in ("alpha", "beta", "bias2", "group", "b_out")})
    a.update(ptrs)
    return lib.gcm_head_chain(a["x"], xs, a["onehots"], hs, a["w1"], w1s, a["b1"], a["w_ma"], a["w2"], w2s, a["alpha"], a["beta"],
                              a["bias2"], a["group"], a["w_out"], a["b_out"], N, I, K, H, G, Cn, kind, factor, slope, a["out"], None)


def _refused(lib, rc, text):
    assert rc == INVALID, rc
    msg = lib.gcm_last_error()
    assert msg and text in msg, msg
    with pytest.raises(RuntimeError, match="gcm_status -1"):
        M.check(rc, "call")


def test_the_caps_are_what_the_header_promises():
    lib = M.lib()
    assert lib.gcm_head_chain_max_hidden() == 512 and lib.gcm_head_chain_max_in() >= 256
    assert modlinear.head_chain_limits() == (lib.gcm_head_chain_max_in(), 512)
    assert lib.gcm_abi_version() == 1


def test_every_argument_rule_is_refused_before_a_device_is_touched(mem):
    lib, _, p = mem
    max_in, max_hidden = lib.gcm_head_chain_max_in(), lib.gcm_head_chain_max_hidden()
    for bad in (6, 0, -4, max_in + 4):
        _refused(lib, _chain(lib, p, I=bad, xs=1024, w1s=1024), b"I must be")
    for bad in (6, 0, -4, max_hidden + 4):
        _refused(lib, _chain(lib, p, H=bad, w2s=1024), b"H must be")
    for bad in (0, -1, 33):
        _refused(lib, _chain(lib, p, K=bad, hs=64), b"K must be")
    _refused(lib, _chain(lib, p, G=0), b"G must be")
    _refused(lib, _chain(lib, p, Cn=2), b"C must be 1 or 3")
    for kind in (-1, 4, 99):
        _refused(lib, _chain(lib, p, kind=kind), b"unknown kind")
    _refused(lib, _chain(lib, p, factor=float("inf")), b"factor")
    for slope in (0.0, -0.2, float("nan")):
        _refused(lib, _chain(lib, p, slope=slope), b"slope")
    for stride in ("xs", "w1s", "w2s"):
        for bad in (6, 0, -8, 4):  # not a multiple of 4, not positive, shorter than the row
            _refused(lib, _chain(lib, p, **{stride: bad}), b"strides")
    for bad in (6, 0, -7):
        _refused(lib, _chain(lib, p, hs=bad), b"onehots_stride")
    for name in ("x", "w1", "b1", "w_ma", "w2", "alpha", "beta", "bias2", "w_out", "b_out", "out"):
        _refused(lib, _chain(lib, p, **{name: p + 4}), b"16-byte")
    _refused(lib, _chain(lib, p, onehots=p + 2), b"4-byte")
    _refused(lib, _chain(lib, p, N=-1), b"N out of range")
    for name in ("x", "onehots", "w1", "b1", "w_ma", "w2", "w_out", "out"):
        _refused(lib, _chain(lib, p, **{name: None}), b"null")


def test_an_empty_problem_and_the_loosest_accepted_arguments_queue_nothing(mem):
    lib, _, p = mem
    assert _chain(lib, p, N=0) == 0
    # a 4-byte aligned onehots pointer with an odd row stride, all optional operands present, the widest shapes, C = 1
    assert _chain(lib, p, N=0, I=lib.gcm_head_chain_max_in(), xs=1024, w1s=1024, H=512, w2s=512, K=32, hs=33, G=5, Cn=1, kind=3,
                  onehots=p + 4, alpha=p, beta=p, bias2=p, b_out=p) == 0
    assert _chain(lib, p, N=0, K=1, hs=1) == 0


def test_head_chain_refuses_what_the_library_does_not_run():
    x, hot, w1, b1, wma, w2, wo = (torch.randn(4, 8), torch.randn(4, 7), torch.randn(8, 8), torch.randn(8), torch.randn(8, 7),
                                   torch.randn(8, 8), torch.randn(3, 8))
    before = modlinear.chain_stats()
    call = lambda *a, kind="rgb": modlinear.head_chain(*a, None, None, None, None, wo, None, kind, 1.0, 0.2)  # noqa: E731
    with pytest.raises(TypeError, match="CUDA"):
        call(x, hot, w1, b1, wma, w2)
    with pytest.raises(TypeError, match="float32"):
        call(x.half(), hot, w1, b1, wma, w2)
    with pytest.raises(ValueError, match="multiples of 4"):
        call(torch.randn(4, 6), hot, torch.randn(8, 6), b1, wma, w2)
    with pytest.raises(ValueError, match="kind"):
        call(x, hot, w1, b1, wma, w2, kind="colour")
    with pytest.raises(ValueError, match="K in 1..32"):
        call(x, torch.randn(4, 40), w1, b1, torch.randn(8, 40), w2)
    assert modlinear.chain_stats() == before and set(before) == {"head_chain_calls"}


# ---- attr_chain on a stand-in models.generator --------------------------------------------------------------------------
def _stand_in():
    """What install() needs of models/generator.py: the two classes with upstream's attribute names.  The head's own forward
    returns a marker, so a test can tell which method ran."""
    class ModLinear(torch.nn.Module):
        pass

    class GaussianAttrMLP(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.factors, self.n_layers, self.n_shared_layers = {"rgb": 2.0}, {"rgb": 1}, 1
            self.act = torch.nn.LeakyReLU(negative_slope=0.2)
            self.fc_m_a, self.fc_1 = torch.nn.Linear(3, 8, bias=False), torch.nn.Linear(4, 8)
            self.fc_2_rgb_0, self.fc_out_rgb = torch.nn.Linear(8, 8), torch.nn.Linear(8, 3)

        def forward(self, pt_feat, onehots, zs):
            return "the module's own method"

    return types.SimpleNamespace(GaussianAttrMLP=GaussianAttrMLP, ModLinear=ModLinear)


def test_install_and_uninstall_alone_are_idempotent_and_restore_the_method():
    G = _stand_in()
    own = G.GaussianAttrMLP.forward
    attr_chain.uninstall(G)  # nothing installed: nothing happens
    assert G.GaussianAttrMLP.forward is own
    attr_chain.install(G)
    bound = G.GaussianAttrMLP.forward
    assert bound is not own
    attr_chain.install(G)
    assert G.GaussianAttrMLP.forward is bound and getattr(G, attr_chain._ORIGINAL) is own
    attr_chain.uninstall(G)
    assert G.GaussianAttrMLP.forward is own and not hasattr(G, attr_chain._ORIGINAL) and not hasattr(G, attr_chain._BOUND)
    attr_chain.uninstall(G)
    assert G.GaussianAttrMLP.forward is own


@pytest.mark.parametrize("first", ["head", "chain"])
@pytest.mark.parametrize("first_out", ["head", "chain"])
def test_install_with_attr_head_in_both_orders_restores_the_original_function_object(first, first_out):
    layer = {"head": attr_head, "chain": attr_chain}
    G = _stand_in()
    own = G.GaussianAttrMLP.forward
    second = "chain" if first == "head" else "head"
    layer[first].install(G)
    under = G.GaussianAttrMLP.forward
    layer[second].install(G)
    top = G.GaussianAttrMLP.forward
    assert under is not own and top is not under
    layer[first].install(G)  # still bound under the other: nothing changes
    assert G.GaussianAttrMLP.forward is top
    head = G.GaussianAttrMLP()
    feat, onehots = torch.randn(1, 5, 4), torch.zeros(1, 5, 3)
    attr_chain.reset_stats()
    attr_head.reset_stats()
    assert head(feat, onehots, None) == "the module's own method"     # through both layers
    assert attr_chain.stats() == {"chain_calls": 0, "passed_on_calls": 1}
    assert attr_head.stats() == {"fused_calls": 0, "original_calls": 1}
    second_out = "chain" if first_out == "head" else "head"
    layer[first_out].uninstall(G)
    assert head(feat, onehots, None) == "the module's own method"
    layer[second_out].uninstall(G)
    assert G.GaussianAttrMLP.forward is own
    for name in (attr_head._ORIGINAL, attr_chain._ORIGINAL, attr_chain._BOUND):
        assert not hasattr(G, name), name
    assert head(feat, onehots, None) == "the module's own method"
    attr_chain.install(G)  # and it binds again afterwards
    assert G.GaussianAttrMLP.forward is not own
    attr_chain.uninstall(G)
    assert G.GaussianAttrMLP.forward is own


def test_cpu_tensors_and_calls_with_gradients_reach_the_method_bound_before_and_are_counted():
    G = _stand_in()
    attr_chain.install(G)
    try:
        attr_chain.reset_stats()
        before = modlinear.chain_stats()
        head = G.GaussianAttrMLP()
        feat, onehots = torch.randn(1, 5, 4), torch.zeros(1, 5, 3)
        zs = {7: {"z": torch.randn(1, 4), "idx": torch.tensor([[True, True, False, True, False]])}}
        assert head(feat, onehots, None) == "the module's own method"          # gradients enabled
        assert attr_chain.stats() == {"chain_calls": 0, "passed_on_calls": 1}
        with torch.no_grad():
            assert head(feat, onehots, None) == "the module's own method"      # CPU tensors
            assert head(feat, onehots, zs) == "the module's own method"
            assert head(feat.double(), onehots.double(), None) == "the module's own method"
        assert attr_chain.stats() == {"chain_calls": 0, "passed_on_calls": 4}
        assert modlinear.chain_stats() == before
        attr_chain.reset_stats()
        assert attr_chain.stats() == {"chain_calls": 0, "passed_on_calls": 0}
    finally:
        attr_chain.uninstall(G)
