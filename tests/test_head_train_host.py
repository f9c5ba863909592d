"""gcm_head_train_* and its Python layers without a GPU (not gpu): the exports and the binding's table agree, every argument
rule of the header comes back as GCM_ERR_INVALID_ARGUMENT with its message on host pointers that are never dereferenced,
before anything is queued; the plan transcribed in tests/head_train_ref.py agrees with the library's plan and workspace
sizes over a sweep; the large GPU cases reach the plan branches they name; attr_head.install(fused_outputs=...) rebinds and
restores, and CPU calls still reach the module's own method."""
import ctypes as C
import types

import pytest
import torch

from gaussiancity_amd import _native_m as M
from gaussiancity_amd import attr_head, modlinear
from head_train_ref import N_GROUPS, N_TWO_TILES, library_plan, plan, workspace_bytes

INVALID = -1  # GCM_ERR_INVALID_ARGUMENT
NAMES = {"gcm_head_train_max_in", "gcm_head_train_pre_floats", "gcm_head_train_plan", "gcm_head_train_workspace_bytes",
         "gcm_head_train_forward", "gcm_head_train_backward"}


@pytest.fixture()
def mem():
    """(the library, a 256-byte aligned address of host memory that no call below reaches the point of using)."""
    buf = (C.c_float * 1024)()
    return M.lib(), buf, (C.addressof(buf) + 255) // 256 * 256


def _keys(p, kinds=(1,), backward=False, packed=False, **over):
    keys = (M.HeadKey * max(len(kinds), 1))()
    for key, kind in zip(keys, kinds):
        key.kind, key.factor, key.h, key.h_stride, key.w, key.b = kind, 0.5, p, 8, p, None
        key.out, key.out_stride = (None if packed or backward else p), 3
        key.dout, key.dout_stride = (p if backward and not packed else None), 3
        key.dh, key.dh_stride, key.dw, key.db = (p, 8, p, p) if backward else (None, 0, None, None)
    for name, value in over.items():   # a stride goes to every key, anything else to the first
        for key in (keys if name in ("h_stride", "dh_stride") else keys[:1]):
            setattr(key, name, value)
    return keys


def _fwd(lib, p, kinds=(1,), packed=False, N=4, I=8, n_keys=None, xyz=True, scales=True, xs=3, ss=3, **over):
    keys = _keys(p, kinds, False, packed, **over)
    return lib.gcm_head_train_forward(keys, len(kinds) if n_keys is None else n_keys, None, N, I, p, p if xyz else None, xs,
                                      p if scales else None, ss, p if packed else None, None)


def _bwd(lib, p, kinds=(1,), packed=False, N=4, I=8, n_keys=None, scales=True, ss=3, dps=14, pre=True, work=True, nbytes=None,
         **over):
    keys = _keys(p, kinds, True, packed, **over)
    n = len(kinds) if n_keys is None else n_keys
    nbytes = workspace_bytes(N, I, max(1, min(n, 4))) if nbytes is None and I % 4 == 0 and 0 < I <= 512 and N >= 0 else (nbytes or 0)
    return lib.gcm_head_train_backward(keys, n, None, N, I, p if pre else None, p if scales else None, ss, p if packed else None,
                                       dps, work if work is not True else p, nbytes, None)


def _refused(lib, rc, text):
    assert rc == INVALID, rc
    msg = lib.gcm_last_error()
    assert msg and text in msg, msg
    with pytest.raises(RuntimeError, match="gcm_status -1"):
        M.check(rc, "call")


def test_the_exports_exist_and_the_table_declares_them():
    lib = M.lib()
    assert NAMES <= set(M.EXPORTED_SYMBOLS) and all(hasattr(lib, n) for n in NAMES)
    assert lib.gcm_head_train_max_in() >= 512 and lib.gcm_head_train_max_in() % 4 == 0
    assert 1 <= lib.gcm_head_train_pre_floats() <= 10
    assert modlinear.head_train_limit() == lib.gcm_head_train_max_in() and lib.gcm_abi_version() == 1
    assert C.sizeof(M.HeadKey) == 104
    assert set(modlinear.head_train_stats()) >= {"forward_calls", "backward_calls"}
    assert set(modlinear.stats()) == {"forward_calls", "backward_calls", "groups_from_masks_calls", "head_out_calls"}
    assert set(attr_head.stats()) == {"fused_calls", "original_calls"} and set(modlinear.chain_stats()) == {"head_chain_calls"}
    assert set(attr_head.output_stats()) == {"head_attrs_calls", "head_points14_calls"}


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_every_argument_rule_is_refused_before_anything_is_queued(mem, call):
    lib, _, p = mem
    limit = lib.gcm_head_train_max_in()
    for kind in (-1, 4, 99):
        _refused(lib, call(lib, p, kinds=(kind,)), b"unknown kind")
    _refused(lib, call(lib, p, kinds=(1, 0, 1)), b"given twice")
    for n in (0, -1, 5):
        _refused(lib, call(lib, p, n_keys=n), b"n_keys must be in 1..4")
    for bad in (6, 0, -4, limit + 4):
        _refused(lib, call(lib, p, I=bad, h_stride=1024), b"I must be a positive multiple of 4")
    _refused(lib, call(lib, p, N=-1), b"N out of range")
    for bad in (6, 0, -8, 4):   # not a multiple of 4, not positive, shorter than the row
        _refused(lib, call(lib, p, h_stride=bad), b"strides")
    _refused(lib, call(lib, p, h=p + 4), b"16-byte")
    _refused(lib, call(lib, p, w=p + 8), b"16-byte")
    _refused(lib, call(lib, p, h=None), b"null h or w")
    _refused(lib, call(lib, p, factor=float("inf")), b"factor")
    # neither form, both forms
    if call is _fwd:
        _refused(lib, call(lib, p, out=None), b"not both and not neither")
        _refused(lib, call(lib, p, packed=True, out=p), b"not both and not neither")
        _refused(lib, call(lib, p, kinds=(1, 3), out=None), b"not both and not neither")
        _refused(lib, call(lib, p, out_stride=2), b"at least C")
        _refused(lib, call(lib, p, kinds=(0, 2), packed=True), b"points14 needs the rgb key")
        _refused(lib, call(lib, p, packed=True, xyz=False), b"points14 needs the rgb key, xyz and scales")
        _refused(lib, call(lib, p, packed=True, scales=False), b"points14 needs the rgb key, xyz and scales")
        _refused(lib, call(lib, p, packed=True, xs=2), b"at least 3")
        _refused(lib, call(lib, p, packed=True, ss=0), b"at least 3")
    else:
        _refused(lib, call(lib, p, dout=None), b"not both and not neither")
        _refused(lib, call(lib, p, packed=True, dout=p), b"not both and not neither")
        _refused(lib, call(lib, p, dout_stride=2), b"at least C")
        _refused(lib, call(lib, p, packed=True, dps=13), b"dpoints_stride")
        _refused(lib, call(lib, p, kinds=(2,), packed=True, scales=False), b"needs scales")
        _refused(lib, call(lib, p, kinds=(2,), packed=True, ss=2), b"needs scales")
        for bad in (6, 0, 4):
            _refused(lib, call(lib, p, dh_stride=bad), b"strides")
        _refused(lib, call(lib, p, dh=p + 4), b"16-byte")
        _refused(lib, call(lib, p, dw=p + 4), b"16-byte")
        _refused(lib, call(lib, p, nbytes=workspace_bytes(4, 8, 1) - 1), b"workspace smaller than gcm_head_train_workspace_bytes")
        _refused(lib, call(lib, p, kinds=(0, 1, 2, 3), nbytes=workspace_bytes(4, 8, 3)), b"workspace smaller")
        _refused(lib, call(lib, p, work=None), b"workspace")
        _refused(lib, call(lib, p, work=p + 16), b"256-byte aligned")
        _refused(lib, call(lib, p, pre=False), b"null pre")


def test_the_sizers_refuse_and_an_empty_forward_queues_nothing(mem):
    lib, _, p = mem
    buf = (C.c_int64 * 8)()
    for bad in (6, 0, lib.gcm_head_train_max_in() + 4):
        assert lib.gcm_head_train_workspace_bytes(4, bad, 1) == 0 and b"I must be" in lib.gcm_last_error()
        _refused(lib, lib.gcm_head_train_plan(4, bad, buf), b"I must be")
    for bad in (0, 5):
        assert lib.gcm_head_train_workspace_bytes(4, 8, bad) == 0 and b"n_keys" in lib.gcm_last_error()
    _refused(lib, lib.gcm_head_train_plan(-1, 8, buf), b"N out of range")
    _refused(lib, lib.gcm_head_train_plan(4, 8, None), b"null plan")
    assert _fwd(lib, p, N=0) == 0 and _fwd(lib, p, N=0, kinds=(0, 1, 2, 3), packed=True, I=512, h_stride=512) == 0
    assert _fwd(lib, p, N=0, h=None, w=None) == 0


def test_the_transcribed_plan_is_the_librarys():
    lib = M.lib()
    for N in (0, 1, 63, 64, 65, 333, 1023, 1024, 1025, 16384, 65536, 65537, N_GROUPS, N_TWO_TILES, 10 ** 6 + 1, 2 ** 31 - 1):
        for I in (4, 8, 52, 512):
            mine = plan(N, I)
            assert library_plan(N, I) == mine, (N, I)
            assert mine["records"] <= 1024 and mine["groups"] <= 16 and mine["groups"] * mine["per"] >= mine["records"]
            assert mine["records"] * mine["tpb"] >= mine["tiles"] > (mine["records"] - 1) * mine["tpb"] or N == 0
            for n_keys in (1, 4):
                assert lib.gcm_head_train_workspace_bytes(N, I, n_keys) == workspace_bytes(N, I, n_keys)
                assert workspace_bytes(N, I, n_keys) >= n_keys * mine["records"] * mine["rec_floats"] * 4


def test_the_large_gpu_cases_reach_the_branches_they_name():
    a, b = plan(N_GROUPS, 8), plan(N_TWO_TILES, 8)
    assert N_GROUPS % 64 and a["tpb"] == 1 and a["groups"] == 14 and a["per"] == 3 and a["levels"] == 2
    assert N_TWO_TILES % 64 and b["tpb"] == 2 and b["tiles"] % 2 == 1 and b["groups"] == 16 and b["levels"] == 2
    assert plan(64, 8)["levels"] == 1 and plan(65, 8)["levels"] == 2


# ---- Python layers --------------------------------------------------------------------------------------------------------
def test_head_attrs_and_head_points14_refuse_what_the_library_does_not_run():
    h, w3, w1 = torch.randn(4, 8), torch.randn(3, 8), torch.randn(1, 8)
    before = modlinear.head_train_stats()
    with pytest.raises(TypeError, match="CUDA"):
        modlinear.head_attrs({"rgb": (h, w3, None, 1.0)})
    with pytest.raises(TypeError, match="float32"):
        modlinear.head_attrs({"rgb": (h.half(), w3, None, 1.0)})
    with pytest.raises(ValueError, match="multiple of 4"):
        modlinear.head_attrs({"rgb": (torch.randn(4, 6), torch.randn(3, 6), None, 1.0)})
    with pytest.raises(ValueError, match="kind"):
        modlinear.head_attrs({"colour": (h, w3, None, 1.0)})
    with pytest.raises(ValueError, match="one to four"):
        modlinear.head_attrs({})
    with pytest.raises(TypeError, match="CUDA"):
        modlinear.head_points14({"opacity": (h, w1, None, 1.0)}, torch.randn(4, 3), torch.randn(4, 3))
    assert modlinear.head_train_stats() == before


def _stand_in():
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


@pytest.mark.parametrize("fused", [False, True])
def test_install_with_the_option_rebinds_restores_and_leaves_cpu_calls_alone(fused):
    G = _stand_in()
    own = G.GaussianAttrMLP.forward
    attr_head.install(G, fused_outputs=fused)
    try:
        bound = G.GaussianAttrMLP.forward
        assert bound is not own
        attr_head.install(G, fused_outputs=not fused)   # idempotent: the first install holds
        assert G.GaussianAttrMLP.forward is bound
        attr_head.reset_stats()
        before = modlinear.head_train_stats()
        head = G.GaussianAttrMLP()
        feat, onehots = torch.randn(1, 5, 4), torch.zeros(1, 5, 3)
        assert head(feat, onehots, None) == "the module's own method"   # CPU tensors, gradients enabled
        with torch.no_grad():
            assert head(feat, onehots, None) == "the module's own method"
        assert attr_head.stats() == {"fused_calls": 0, "original_calls": 2}
        assert attr_head.output_stats() == {"head_attrs_calls": 0, "head_points14_calls": 0}
        assert modlinear.head_train_stats() == before
        with pytest.raises(ValueError, match="not one the HIP output layers take"):
            attr_head.gaussian_points(head, feat, onehots, None, torch.zeros(1, 5, 3), torch.ones(1, 5, 3))
    finally:
        attr_head.uninstall(G)
    assert G.GaussianAttrMLP.forward is own and not hasattr(G, attr_head._ORIGINAL)
    with pytest.raises(RuntimeError, match="install"):
        attr_head.gaussian_points(G.GaussianAttrMLP(), torch.randn(1, 5, 4), torch.zeros(1, 5, 3), None, torch.zeros(1, 5, 3),
                                  torch.ones(1, 5, 3))
