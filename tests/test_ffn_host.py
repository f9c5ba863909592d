"""The feed-forward operator of libgcm_hip.so and its two Python layers without a GPU (not gpu): the four gcm_ffn_* names are
in the header, the binding table and the library's dynamic symbols, the capability query answers at least 128, every
argument error of the header comes back as GCM_ERR_INVALID_ARGUMENT with a message before a device is touched, the workspace
query is monotone, and point_ffn.install / uninstall rebind and restore Block.forward of a stand-in models.pt_v3 whose own
method runs (and is counted) for everything the operator does not compute."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest
import torch

from gaussiancity_amd import _native_m as M
from gaussiancity_amd import ffn, point_block, point_ffn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1  # GCM_ERR_INVALID_ARGUMENT
NAMES = {"gcm_ffn_max_channels", "gcm_ffn_forward", "gcm_ffn_backward_workspace_bytes", "gcm_ffn_backward"}


def test_the_four_names_are_in_the_header_the_binding_and_the_library():
    lib = M.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gcm.h")).read(), flags=re.S)
    assert NAMES <= set(re.findall(r"\b(gcm_[a-z_]+)\s*\(", header))
    assert NAMES <= set(M.EXPORTED_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", M.LIB_PATH]).decode()
    assert NAMES <= set(re.findall(r" T (gcm_[a-z_]+)", out))
    assert not [name for name in NAMES if getattr(lib, name).argtypes is None]
    assert lib.gcm_abi_version() == 1


def test_the_fused_kernels_hold_at_least_128_channels():
    assert M.lib().gcm_ffn_max_channels() >= 128 and ffn.max_channels() == M.lib().gcm_ffn_max_channels()


@pytest.fixture()
def mem():
    """(the library, a 256-byte aligned address of host memory that no call below reaches the point of using)."""
    buf = (C.c_float * 1024)()
    return M.lib(), buf, (C.addressof(buf) + 255) // 256 * 256


def _forward(lib, p, xs=8, ys=8, N=4, Cn=8, Hd=16, eps=1e-5, a=None, mean=None, rstd=None, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    return lib.gcm_ffn_forward(g("x"), xs, g("ln_w"), g("ln_b"), eps, g("w1"), g("b1"), g("w2"), g("b2"), None, N, Cn, Hd,
                               g("y"), ys, mean, rstd, a, None)


def _backward(lib, p, xs=8, dys=8, dxs=8, N=4, Cn=8, Hd=16, work="p", bytes_=None, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    need = lib.gcm_ffn_backward_workspace_bytes(N, Cn, Hd) if bytes_ is None else bytes_
    return lib.gcm_ffn_backward(g("x"), xs, p, p, g("a"), g("dy"), dys, None, g("ln_w"), g("ln_b"), g("w1"), g("w2"), N, Cn, Hd,
                                g("dx"), dxs, g("dln_w"), g("dln_b"), g("dw1"), g("db1"), g("dw2"), g("db2"),
                                p if work == "p" else work, need, None)


def _refused(lib, rc, text):
    assert rc == INVALID, rc
    msg = lib.gcm_last_error()
    assert msg and text in msg, msg
    with pytest.raises(RuntimeError, match="gcm_status -1"):
        M.check(rc, "call")


def test_forward_argument_errors_come_back_before_a_device_is_touched(mem):
    lib, _, p = mem
    limit = lib.gcm_ffn_max_channels()
    for bad in (6, 0, -4):
        _refused(lib, _forward(lib, p, Cn=bad), b"C must be")
        _refused(lib, _forward(lib, p, Hd=bad), b"Hd must be")
    _refused(lib, _forward(lib, p, Cn=limit + 4, xs=limit + 4, ys=limit + 4), b"C above")
    _refused(lib, _forward(lib, p, Hd=4 * limit + 4), b"Hd above")
    for stride in ("xs", "ys"):
        for bad in (6, 0, -8, 4):  # not a multiple of 4, not positive, shorter than the row
            _refused(lib, _forward(lib, p, **{stride: bad}), b"strides")
    for name in ("x", "ln_w", "ln_b", "w1", "b1", "w2", "b2", "y"):
        _refused(lib, _forward(lib, p, **{name: p + 4}), b"16-byte")
    _refused(lib, _forward(lib, p, a=p + 4, mean=p, rstd=p), b"16-byte")
    _refused(lib, _forward(lib, p, N=-1), b"N out of range")
    _refused(lib, _forward(lib, p, eps=-1.0), b"eps")
    _refused(lib, _forward(lib, p, x=None), b"null")
    _refused(lib, _forward(lib, p, a=p), b"mean and rstd")      # the stored pre-activation needs the statistics beside it
    _refused(lib, _forward(lib, p, mean=p), b"mean and rstd")
    assert _forward(lib, p, N=0) == 0  # an empty problem is fine and queues nothing


def test_backward_argument_errors_and_a_short_null_or_misaligned_workspace(mem):
    lib, _, p = mem
    limit = lib.gcm_ffn_max_channels()
    _refused(lib, _backward(lib, p, Cn=10, bytes_=1 << 20), b"C must be")
    _refused(lib, _backward(lib, p, Hd=2, bytes_=1 << 20), b"Hd must be")
    _refused(lib, _backward(lib, p, Cn=limit + 4, xs=limit + 4, dys=limit + 4, dxs=limit + 4, bytes_=1 << 30), b"C above")
    for stride in ("xs", "dys", "dxs"):
        for bad in (10, 4, 0):
            _refused(lib, _backward(lib, p, **{stride: bad}), b"strides")
    for name in ("x", "a", "dy", "ln_w", "ln_b", "w1", "w2", "dx", "dln_w", "dln_b", "dw1", "db1", "dw2", "db2"):
        _refused(lib, _backward(lib, p, **{name: p + 8}), b"16-byte")
    need = lib.gcm_ffn_backward_workspace_bytes(4, 8, 16)
    assert need > 0
    _refused(lib, _backward(lib, p, bytes_=need - 1), b"workspace smaller")
    _refused(lib, _backward(lib, p, work=None), b"workspace smaller")
    _refused(lib, _backward(lib, p, work=p + 16), b"256-byte")
    _refused(lib, _backward(lib, p, x=None), b"null")


def test_workspace_query_is_monotone_in_the_rows_and_refuses_bad_shapes():
    lib = M.lib()
    for Cn, Hd in ((4, 4), (32, 128), (48, 40), (128, 512)):
        sizes = [lib.gcm_ffn_backward_workspace_bytes(n, Cn, Hd) for n in (0, 1, 63, 64, 65, 130, 333, 4096, 4160, 65536, 262144)]
        assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[0] % 256 == 0 and sizes[-1] >= 262144 * Hd * 4, sizes
    assert lib.gcm_ffn_backward_workspace_bytes(10, 6, 8) == 0 and b"C must be" in lib.gcm_last_error()
    assert lib.gcm_ffn_backward_workspace_bytes(10, 8, 6) == 0 and b"Hd must be" in lib.gcm_last_error()
    assert lib.gcm_ffn_backward_workspace_bytes(10, 132, 512) == 0 and b"C above" in lib.gcm_last_error()
    assert lib.gcm_ffn_backward_workspace_bytes(-1, 8, 8) == 0 and lib.gcm_last_error()


def test_the_operator_refuses_what_the_library_does_not_run():
    C_, Hd = 8, 16
    args = [torch.randn(4, C_), torch.ones(C_), torch.zeros(C_), 1e-5, torch.randn(Hd, C_), torch.zeros(Hd), torch.randn(C_, Hd),
            torch.zeros(C_)]
    with pytest.raises(TypeError, match="CUDA"):
        ffn.layernorm_mlp_residual(*args)
    with pytest.raises(TypeError, match="float32"):
        ffn.layernorm_mlp_residual(args[0].half(), *args[1:])
    with pytest.raises(ValueError, match="multiples of 4"):
        ffn.layernorm_mlp_residual(torch.randn(4, 6), torch.ones(6), torch.zeros(6), 1e-5, torch.randn(Hd, 6), *args[5:])
    with pytest.raises(ValueError, match=r"x must be \[N, C\]"):
        ffn.layernorm_mlp_residual(args[0][0], *args[1:])
    assert set(ffn.stats()) == {"forward_calls", "backward_calls"}


def test_torchs_own_float32_run_handles_a_constant_row_and_rows_of_very_different_scale():
    """The inputs of test_ffn_gpu.py's special-rows case are fair: torch's float32 formulation on the CPU stays within
    2^-19 of the largest element of the float64 result in every tensor -- sqrt(512) * 2^-24 = 1.35e-6 is the random-walk
    rounding of the longest sum there (512 hidden features), rounded up to a power of two -- so nothing in them (rstd =
    1 / sqrt(eps) on the constant row, a factor 1e6 between two rows) is beyond float32."""
    import test_ffn_gpu as G
    for C_, Hd in G.SHAPES:
        inp = G.special_rows(G.make_inputs(65, C_, Hd, 300))
        assert float(inp["x"][3].var(unbiased=False)) == 0.0
        fig = G.figures(G.run(G.torch_ops, inp, "cpu", torch.float32), G.run(G.torch_ops, inp, "cpu", torch.float64))
        assert all(v <= 2.0 ** -19 for v in fig.values()), (C_, Hd, fig)


# ---- point_ffn on a stand-in models.pt_v3 -----------------------------------------------------------------------------------
def _stand_in():
    """What install() needs of models/pt_v3.py, written for this test: a Block that holds its sub-modules under
    upstream's names.  Its own forward returns a marker, so a test can tell which method ran."""
    class Seq(torch.nn.Sequential):
        pass

    class MLP(torch.nn.Module):
        def __init__(self, c, hidden, act):
            super().__init__()
            self.fc1, self.act, self.fc2 = torch.nn.Linear(c, hidden), act, torch.nn.Linear(hidden, c)

    class Block(torch.nn.Module):
        def __init__(self, c=8, pre_norm=True, act=None):
            super().__init__()
            self.pre_norm = pre_norm
            self.cpe, self.norm1, self.attn = Seq(torch.nn.Identity()), Seq(torch.nn.Identity()), torch.nn.Identity()
            self.norm2 = Seq(torch.nn.LayerNorm(c))
            self.mlp = Seq(MLP(c, 4 * c, act if act is not None else torch.nn.GELU()))
            self.drop_path = Seq(torch.nn.Identity())

        def forward(self, point):
            return "the module's own method"

    return types.SimpleNamespace(Block=Block)


def test_install_and_uninstall_are_idempotent_and_restore_the_method():
    P = _stand_in()
    own = P.Block.forward
    point_ffn.uninstall(P)  # nothing installed: nothing happens
    assert P.Block.forward is own
    point_ffn.install(P)
    bound = P.Block.forward
    assert bound is not own
    point_ffn.install(P)
    st = point_block.state(P)
    assert P.Block.forward is bound and st.bound is bound and st.original is own and st.ffn == (ffn.max_channels(), False)
    point_ffn.uninstall(P)
    assert P.Block.forward is own and point_block.state(P) is None
    assert not [n for n in vars(P) if n.startswith("_gaussiancity_amd")]
    point_ffn.uninstall(P)
    assert P.Block.forward is own


class _FakeCuda:
    """A feature tensor's stand-in that says it is on the GPU: the checks that come after the device are reached here."""
    is_cuda = True

    def __init__(self, n, c, dtype=torch.float32):
        self.shape, self.dtype = (n, c), dtype

    def dim(self):
        return 2


def test_what_the_operator_does_not_compute_reaches_the_modules_own_method_and_is_counted():
    P = _stand_in()
    point_ffn.install(P)
    try:
        point_ffn.reset_stats()
        mine = "the module's own method"
        point = types.SimpleNamespace(feat=torch.randn(5, 8))
        assert P.Block()(point) == mine                                                   # CPU tensors
        assert P.Block(pre_norm=False)(types.SimpleNamespace(feat=_FakeCuda(5, 8))) == mine
        assert P.Block(act=torch.nn.GELU(approximate="tanh"))(types.SimpleNamespace(feat=_FakeCuda(5, 8))) == mine
        assert P.Block(act=torch.nn.ReLU())(types.SimpleNamespace(feat=_FakeCuda(5, 8))) == mine
        torch.set_autocast_enabled(True)  # (the context manager switches itself off where no GPU is visible)
        try:
            assert P.Block()(types.SimpleNamespace(feat=_FakeCuda(5, 8))) == mine          # an active autocast
        finally:
            torch.set_autocast_enabled(False)
        wide = ffn.max_channels() + 4
        assert P.Block(c=wide)(types.SimpleNamespace(feat=_FakeCuda(5, wide))) == mine    # a C above the limit
        assert P.Block()(types.SimpleNamespace(feat=_FakeCuda(5, 8, torch.float16))) == mine
        assert point_ffn.stats() == {"fused_calls": 0, "original_calls": 7}
        # the stand-in that says it is on the GPU passes every check when nothing is in the way: the cases above were
        # turned away by what they name, not by the stand-in
        assert point_ffn._parts(P.Block(), types.SimpleNamespace(feat=_FakeCuda(5, 8))) is not None
        point_ffn.reset_stats()
        assert point_ffn.stats() == {"fused_calls": 0, "original_calls": 0}
    finally:
        point_ffn.uninstall(P)
