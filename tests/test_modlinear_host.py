"""libgcm_hip.so and its two Python layers without a GPU (not gpu): the library loads and exports exactly what
include/gcm.h declares, every argument error of the header comes back as GCM_ERR_INVALID_ARGUMENT with a message before
a device is touched, the workspace query is monotone, and attr_head.install / uninstall rebind and restore the method of
a stand-in models.generator whose own method runs (and is counted) for CPU tensors and for zs None."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest
import torch

from gaussiancity_amd import _native_m as M
from gaussiancity_amd import attr_head, modlinear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1  # GCM_ERR_INVALID_ARGUMENT


def test_header_binding_and_library_name_the_same_functions():
    lib = M.lib()
    header = open(os.path.join(ROOT, "include", "gcm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(gcm_[a-z_]+)\s*\(", src))
    assert declared == set(M.EXPORTED_SYMBOLS), (sorted(declared), M.EXPORTED_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", M.LIB_PATH]).decode()
    assert set(re.findall(r" T (gcm_[a-z_]+)", out)) == declared
    assert not [name for name in M.EXPORTED_SYMBOLS if getattr(lib, name).argtypes is None]
    assert b"gfx950" in open(M.LIB_PATH, "rb").read()
    kinds = re.search(r"enum gcm_kind \{(.*?)\}", src, flags=re.S).group(1)
    assert {k.lower(): int(v) for k, v in re.findall(r"GCM_([A-Z]+) = (\d+)", kinds)} == M.KINDS
    assert modlinear.KINDS == ("xyz", "rgb", "scale", "opacity") and modlinear.dtypes() == (torch.float32,)


def test_abi_number_is_one():
    header = open(os.path.join(ROOT, "include", "gcm.h")).read()
    assert M.lib().gcm_abi_version() == M.ABI_VERSION == 1 == int(re.search(r"#define GCM_ABI_VERSION (\d+)", header).group(1))


@pytest.fixture()
def mem():
    """(the library, a 256-byte aligned address of host memory that no call below reaches the point of using)."""
    buf = (C.c_float * 1024)()
    return M.lib(), buf, (C.addressof(buf) + 255) // 256 * 256


def _forward(lib, p, x=None, xs=8, w=None, ws=8, alpha=None, beta=None, bias=None, N=4, I=8, O=8, G=1, slope=0.2, y=None,
             ys=8):
    pick = lambda v: p if v is None else v  # noqa: E731
    return lib.gcm_modlinear_forward(pick(x), xs, pick(w), ws, alpha, beta, bias, None, N, I, O, G, slope, pick(y), ys, None)


def _backward(lib, p, N=4, I=8, O=8, G=1, xs=8, ys=8, dys=8, ws=8, dxs=8, x=None, dx=None, dw=None, work=None, bytes_=None):
    pick = lambda v: p if v is None else v  # noqa: E731
    need = lib.gcm_modlinear_backward_workspace_bytes(N, I, O, G) if bytes_ is None else bytes_
    return lib.gcm_modlinear_backward(pick(x), xs, p, ys, p, dys, p, ws, None, None, N, I, O, G, 0.2, pick(dx), dxs, pick(dw),
                                      None, None, None, pick(work), need, None)


def _refused(lib, rc, text):
    assert rc == INVALID, rc
    msg = lib.gcm_last_error()
    assert msg and text in msg, msg
    with pytest.raises(RuntimeError, match="gcm_status -1"):
        M.check(rc, "call")


def test_forward_argument_errors_come_back_before_a_device_is_touched(mem):
    lib, _, p = mem
    for bad in (6, 0, -4):
        _refused(lib, _forward(lib, p, I=bad), b"I must be")
        _refused(lib, _forward(lib, p, O=bad), b"O must be")
    for stride in ("xs", "ws", "ys"):
        for bad in (6, 0, -8, 4):  # not a multiple of 4, not positive, shorter than the row
            _refused(lib, _forward(lib, p, **{stride: bad}), b"strides")
    for name in ("x", "w", "alpha", "beta", "bias", "y"):
        _refused(lib, _forward(lib, p, **{name: p + 4}), b"16-byte")
    _refused(lib, _forward(lib, p, N=-1), b"N out of range")
    _refused(lib, _forward(lib, p, G=0), b"G must be")
    _refused(lib, _forward(lib, p, slope=0.0), b"slope")
    _refused(lib, lib.gcm_modlinear_forward(None, 8, p, 8, None, None, None, None, 4, 8, 8, 1, 0.2, p, 8, None), b"null")
    assert _forward(lib, p, N=0) == 0  # an empty problem is fine and queues nothing


def test_backward_argument_errors_and_a_short_workspace(mem):
    lib, _, p = mem
    _refused(lib, _backward(lib, p, I=10, bytes_=1 << 20), b"I must be")
    _refused(lib, _backward(lib, p, O=2, bytes_=1 << 20), b"O must be")
    for stride in ("xs", "ys", "dys", "ws", "dxs"):
        _refused(lib, _backward(lib, p, **{stride: 10}), b"strides")
    for name in ("x", "dx", "dw"):
        _refused(lib, _backward(lib, p, **{name: p + 8}), b"16-byte")
    need = lib.gcm_modlinear_backward_workspace_bytes(4, 8, 8, 1)
    assert need > 0
    _refused(lib, _backward(lib, p, bytes_=need - 1), b"workspace smaller")
    _refused(lib, _backward(lib, p, work=p + 16), b"256-byte")
    _refused(lib, lib.gcm_modlinear_backward(p, 8, p, 8, p, 8, p, 8, None, None, 4, 8, 8, 1, 0.2, p, 8, p, None, None, None,
                                             None, need, None), b"workspace smaller")


def test_head_out_and_groups_from_masks_argument_errors(mem):
    lib, _, p = mem

    def head(f=p, fs=8, w=p, N=4, I=8, Cn=3, kind=1):
        return lib.gcm_head_out(f, fs, w, None, None, N, I, Cn, kind, 0.5, p, None)

    for kind in (-1, 4, 99):
        _refused(lib, head(kind=kind), b"unknown kind")
    _refused(lib, head(I=6), b"I must be")
    _refused(lib, head(Cn=2), b"C must be 1 or 3")
    _refused(lib, head(fs=6), b"strides")
    _refused(lib, head(f=p + 4), b"16-byte")
    _refused(lib, head(w=p + 4), b"16-byte")
    assert head(N=0) == 0
    _refused(lib, lib.gcm_groups_from_masks(p, 2, -1, p, None), b"N out of range")
    _refused(lib, lib.gcm_groups_from_masks(p, -1, 4, p, None), b"G must be")
    _refused(lib, lib.gcm_groups_from_masks(None, 2, 4, p, None), b"null masks")
    _refused(lib, lib.gcm_groups_from_masks(p, 2, 4, None, None), b"null group")
    assert lib.gcm_groups_from_masks(None, 0, 0, None, None) == 0


def test_workspace_query_is_monotone_in_the_rows_and_refuses_bad_shapes():
    lib = M.lib()
    for I, O, G in ((4, 4, 1), (20, 36, 5), (512, 512, 16)):
        sizes = [lib.gcm_modlinear_backward_workspace_bytes(n, I, O, G) for n in (0, 1, 63, 64, 65, 130, 333, 4096, 65536)]
        assert sizes == sorted(sizes) and sizes[0] % 256 == 0 and sizes[-1] >= 65536 * I * 4, sizes
    assert lib.gcm_modlinear_backward_workspace_bytes(10, 6, 8, 1) == 0 and b"I must be" in lib.gcm_last_error()
    assert lib.gcm_modlinear_backward_workspace_bytes(-1, 8, 8, 1) == 0 and lib.gcm_last_error()


# ---- attr_head on a stand-in models.generator ---------------------------------------------------------------------------
def _stand_in():
    """What install() needs of models/generator.py, written for this test: the two classes with upstream's attribute
    names.  The head's own forward returns a marker, so a test can tell which method ran."""
    class ModLinear(torch.nn.Module):
        def __init__(self, in_features, out_features, style_features):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.randn(out_features, in_features))
            self.bias, self.mod_bias, self.output_mode = None, True, True
            self.weight_alpha = torch.nn.Parameter(torch.randn(in_features, style_features))
            self.bias_alpha = torch.nn.Parameter(torch.ones(in_features))
            self.weight_beta = torch.nn.Parameter(torch.randn(out_features, style_features))
            self.bias_beta = torch.nn.Parameter(torch.zeros(out_features))

        def forward(self, x, z):
            raise AssertionError("the stand-in ModLinear does not compute")

    class GaussianAttrMLP(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.factors, self.n_layers, self.n_shared_layers = {"rgb": 2.0}, {"rgb": 1}, 1
            self.act = torch.nn.LeakyReLU(negative_slope=0.2)
            self.fc_m_a, self.fc_1 = torch.nn.Linear(3, 8, bias=False), torch.nn.Linear(4, 8)
            self.fc_2_rgb_0, self.fc_out_rgb = ModLinear(8, 8, 4), torch.nn.Linear(8, 3)

        def forward(self, pt_feat, onehots, zs):
            return "the module's own method"

    return types.SimpleNamespace(GaussianAttrMLP=GaussianAttrMLP, ModLinear=ModLinear)


def test_install_and_uninstall_are_idempotent_and_restore_the_method():
    G = _stand_in()
    own = G.GaussianAttrMLP.forward
    attr_head.uninstall(G)  # nothing installed: nothing happens
    assert G.GaussianAttrMLP.forward is own
    attr_head.install(G)
    bound = G.GaussianAttrMLP.forward
    assert bound is not own
    attr_head.install(G)
    assert G.GaussianAttrMLP.forward is bound and getattr(G, attr_head._ORIGINAL) is own
    attr_head.uninstall(G)
    assert G.GaussianAttrMLP.forward is own and not hasattr(G, attr_head._ORIGINAL)
    attr_head.uninstall(G)
    assert G.GaussianAttrMLP.forward is own


def test_cpu_tensors_and_a_head_without_codes_reach_the_modules_own_method_and_are_counted():
    G = _stand_in()
    attr_head.install(G)
    try:
        attr_head.reset_stats()
        head = G.GaussianAttrMLP()
        feat, onehots = torch.randn(1, 5, 4), torch.zeros(1, 5, 3)
        zs = {7: {"z": torch.randn(1, 4), "idx": torch.tensor([[True, True, False, True, False]])}}
        assert head(feat, onehots, None) == "the module's own method"
        assert attr_head.stats() == {"fused_calls": 0, "original_calls": 1}
        assert head(feat, onehots, zs) == "the module's own method"      # CPU tensors
        assert head(feat.double(), onehots.double(), zs) == "the module's own method"
        assert head(feat.expand(2, 5, 4), onehots.expand(2, 5, 3), zs) == "the module's own method"
        assert attr_head.stats() == {"fused_calls": 0, "original_calls": 4}
        attr_head.reset_stats()
        assert attr_head.stats() == {"fused_calls": 0, "original_calls": 0}
    finally:
        attr_head.uninstall(G)


def test_modlinear_refuses_what_the_library_does_not_run():
    x, w = torch.randn(4, 8), torch.randn(8, 8)
    with pytest.raises(TypeError, match="CUDA"):
        modlinear.modulated_linear(x, w)
    with pytest.raises(TypeError, match="float32"):
        modlinear.modulated_linear(x.half(), w.half())
    with pytest.raises(ValueError, match="multiples of 4"):
        modlinear.modulated_linear(torch.randn(4, 6), torch.randn(8, 6))
    with pytest.raises(ValueError, match="kind"):
        modlinear.head_out(x, torch.randn(3, 8), None, None, "colour", 1.0)
    assert set(modlinear.stats()) == {"forward_calls", "backward_calls", "groups_from_masks_calls", "head_out_calls"}
