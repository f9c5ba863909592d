"""The Block-middle operators of libgcm_hip.so and their two Python layers without a GPU (not gpu): the seven gcm_mid_* names
are in the header, the binding table and the library's dynamic symbols, the capability query answers at least 128, every
argument error of the header comes back as GCM_ERR_INVALID_ARGUMENT with a message before a device is touched, an empty
problem returns 0, the workspace query agrees with the transcribed plan of tests/mid_plans.py; mid's operators refuse what
the library does not run; point_mid.install / uninstall turn the middle on and off on a stand-in models.pt_v3, install
point_front when it is not bound and leave it otherwise, in both orders with point_ffn; torch's own float32 run is fair on
the inputs of tests/test_mid_gpu.py."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest
import torch

import mid_plans as P
import mid_ref as R
from gaussiancity_amd import _native_m as M
from gaussiancity_amd import front, mid, point_block, point_ffn, point_front, point_mid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1  # GCM_ERR_INVALID_ARGUMENT
NAMES = {"gcm_mid_max_channels", "gcm_mid_slot_plan", "gcm_mid_gather_forward", "gcm_mid_gather_backward", "gcm_mid_forward",
         "gcm_mid_backward_workspace_bytes", "gcm_mid_backward"}


def test_the_seven_names_are_in_the_header_the_binding_and_the_library():
    lib = M.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gcm.h")).read(), flags=re.S)
    assert NAMES <= set(re.findall(r"\b(gcm_[a-z_]+)\s*\(", header))
    assert NAMES <= set(M.EXPORTED_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", M.LIB_PATH]).decode()
    assert NAMES <= set(re.findall(r" T (gcm_[a-z_]+)", out))
    assert not [name for name in NAMES if getattr(lib, name).argtypes is None]
    assert lib.gcm_abi_version() == 1


def test_the_fused_kernels_hold_at_least_128_channels():
    assert M.lib().gcm_mid_max_channels() >= 128 and mid.max_channels() == M.lib().gcm_mid_max_channels()


@pytest.fixture()
def mem():
    """(the library, a 256-byte aligned address of host memory that no call below reaches the point of using)."""
    buf = (C.c_float * 1024)()
    return M.lib(), buf, (C.addressof(buf) + 255) // 256 * 256


def _refused(lib, rc, text):
    assert rc == INVALID, rc
    msg = lib.gcm_last_error()
    assert msg and text in msg, msg
    with pytest.raises(RuntimeError, match="gcm_status -1"):
        M.check(rc, "call")


def _plan(lib, p, T=6, N=4, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    return lib.gcm_mid_slot_plan(g("order"), T, g("inverse"), N, g("extra"), None)


def _gather(lib, p, xs=8, T=6, W=8, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    return lib.gcm_mid_gather_forward(g("x"), xs, g("order"), T, W, g("y"), None)


def _gather_bwd(lib, p, dys=8, N=4, W=8, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    return lib.gcm_mid_gather_backward(g("dy"), dys, g("inverse"), g("extra"), N, W, g("dx"), None)


def _forward(lib, p, as_=8, xs=8, ys=8, N=4, Cn=8, row_scale=None, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    return lib.gcm_mid_forward(g("a"), as_, g("inverse"), g("x"), xs, g("wp"), g("bp"), row_scale, N, Cn, g("y"), ys, None)


def _backward(lib, p, as_=8, dys=8, N=4, T=6, Cn=8, work="p", bytes_=None, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    need = lib.gcm_mid_backward_workspace_bytes(N, Cn) if bytes_ is None else bytes_
    return lib.gcm_mid_backward(g("a"), as_, g("inverse"), g("extra"), g("dy"), dys, g("wp"), None, N, T, Cn, g("da"), g("dwp"),
                                g("dbp"), p if work == "p" else work, need, None)


def test_plan_and_gather_argument_errors_come_back_before_a_device_is_touched(mem):
    lib, _, p = mem
    _refused(lib, _plan(lib, p, N=-1), b"N out of range")
    _refused(lib, _plan(lib, p, N=1 << 31, T=1 << 31), b"N out of range")
    _refused(lib, _plan(lib, p, T=-1, N=0), b"T out of range")
    _refused(lib, _plan(lib, p, T=1 << 31), b"T out of range")
    _refused(lib, _plan(lib, p, T=3), b"T below N")
    for name in ("order", "inverse", "extra"):
        _refused(lib, _plan(lib, p, **{name: None}), b"null")
    _refused(lib, _plan(lib, p, order=p + 4), b"8-byte")
    _refused(lib, _plan(lib, p, extra=p + 2), b"4-byte")
    assert _plan(lib, p, N=0, T=0) == 0 and _plan(lib, p, N=0, T=5) == 0    # no row: nothing to plan, nothing queued

    for bad in (6, 0, -4):
        _refused(lib, _gather(lib, p, W=bad), b"W must be")
        _refused(lib, _gather_bwd(lib, p, W=bad), b"W must be")
    _refused(lib, _gather(lib, p, T=-1), b"T out of range")
    _refused(lib, _gather(lib, p, T=1 << 31), b"T out of range")
    _refused(lib, _gather_bwd(lib, p, N=-1), b"N out of range")
    _refused(lib, _gather_bwd(lib, p, N=1 << 31), b"N out of range")
    for bad in (6, 0, -8, 4):
        _refused(lib, _gather(lib, p, xs=bad), b"strides")
        _refused(lib, _gather_bwd(lib, p, dys=bad), b"strides")
    for name in ("x", "y"):
        _refused(lib, _gather(lib, p, **{name: p + 4}), b"16-byte")
        _refused(lib, _gather(lib, p, **{name: None}), b"null")
    for name in ("dy", "dx"):
        _refused(lib, _gather_bwd(lib, p, **{name: p + 4}), b"16-byte")
        _refused(lib, _gather_bwd(lib, p, **{name: None}), b"null")
    _refused(lib, _gather(lib, p, order=None), b"null")
    _refused(lib, _gather_bwd(lib, p, inverse=None), b"null")
    _refused(lib, _gather_bwd(lib, p, extra=None), b"null")
    assert _gather(lib, p, T=0) == 0 and _gather_bwd(lib, p, N=0) == 0


def test_forward_and_backward_argument_errors_and_a_short_null_or_misaligned_workspace(mem):
    lib, _, p = mem
    limit = lib.gcm_mid_max_channels()
    wide = limit + 4
    for bad in (6, 0, -4):
        _refused(lib, _forward(lib, p, Cn=bad), b"C must be")
        _refused(lib, _backward(lib, p, Cn=bad, bytes_=1 << 20), b"C must be")
    _refused(lib, _forward(lib, p, Cn=wide, as_=wide, xs=wide, ys=wide), b"C above")
    _refused(lib, _backward(lib, p, Cn=wide, as_=wide, dys=wide, bytes_=1 << 30), b"C above")
    _refused(lib, _forward(lib, p, N=-1), b"N out of range")
    _refused(lib, _backward(lib, p, N=-1, bytes_=1 << 20), b"N out of range")
    _refused(lib, _backward(lib, p, T=-1, N=0), b"T out of range")
    _refused(lib, _backward(lib, p, T=1 << 31), b"T out of range")
    _refused(lib, _backward(lib, p, T=3), b"T below N")
    for stride in ("as_", "xs", "ys"):
        for bad in (6, 0, -8, 4):
            _refused(lib, _forward(lib, p, **{stride: bad}), b"strides")
    for stride in ("as_", "dys"):
        for bad in (10, 4, 0):
            _refused(lib, _backward(lib, p, **{stride: bad}), b"strides")
    for name in ("a", "x", "wp", "bp", "y"):
        _refused(lib, _forward(lib, p, **{name: p + 4}), b"16-byte")
        _refused(lib, _forward(lib, p, **{name: None}), b"null")
    _refused(lib, _forward(lib, p, inverse=None), b"null")
    _refused(lib, _forward(lib, p, inverse=p + 4), b"8-byte")
    for name in ("a", "dy", "wp", "da", "dwp", "dbp"):
        _refused(lib, _backward(lib, p, **{name: p + 8}), b"16-byte")
    for name in ("a", "inverse", "extra", "dy", "wp"):
        _refused(lib, _backward(lib, p, **{name: None}), b"null")
    need = lib.gcm_mid_backward_workspace_bytes(4, 8)
    assert need > 0
    _refused(lib, _backward(lib, p, bytes_=need - 1), b"workspace smaller")
    _refused(lib, _backward(lib, p, work=None), b"workspace smaller")
    _refused(lib, _backward(lib, p, work=p + 16), b"256-byte")
    assert _forward(lib, p, N=0) == 0  # an empty problem is fine and queues nothing


def test_the_transcribed_plan_carves_what_the_library_asks_for():
    lib = M.lib()
    for Cn in (4, 32, 36, 48, 64, 68, 100, 128):
        sizes = []
        for N in (0, 1, 63, 64, 65, 130, 333, 4095, 4096, 4097, 8193, 65536, 262144):
            p = P.mid_plan(N, Cn)
            assert lib.gcm_mid_backward_workspace_bytes(N, Cn) == p["total"], (N, Cn, p)
            assert p["total"] % 256 == 0 and p["total"] > 0 and p["sw"] <= P.MAX_SLICES and p["launches"] == 3
            rows = sum(max(min((s + 1) * p["per"], N) - s * p["per"], 0) for s in range(p["sw"]))
            assert rows == N and p["per"] % P.KC == 0, (N, Cn, p)
            sizes.append(p["total"])
        assert sizes == sorted(sizes) and sizes[-1] == sizes[-2]          # bounded: the slices stop at their cap
    assert P.mid_plan(4097, 128)["sw"] == 64 and P.mid_plan(4097, 128)["empty_slices"] == 12
    assert P.mid_plan(10, 8, da=False)["launches"] == 2 and P.mid_plan(10, 8, params=False)["launches"] == 1
    assert lib.gcm_mid_backward_workspace_bytes(10, 6) == 0 and b"C must be" in lib.gcm_last_error()
    assert lib.gcm_mid_backward_workspace_bytes(10, 132) == 0 and b"C above" in lib.gcm_last_error()
    assert lib.gcm_mid_backward_workspace_bytes(-1, 8) == 0 and lib.gcm_last_error()


# ---- the Python operators -----------------------------------------------------------------------------------------------------
def test_the_operators_refuse_what_the_library_does_not_run():
    inp = R.make_inputs(5, 2, 8, 1)
    order, inverse, extra = inp["order"], inp["inverse"], inp["extra"]
    with pytest.raises(TypeError, match="CUDA"):
        mid.slot_plan(order, inverse)
    with pytest.raises(TypeError, match="int64"):
        mid.slot_plan(order.int(), inverse)
    with pytest.raises(ValueError, match="T >= N"):
        mid.slot_plan(order[:3], inverse)
    with pytest.raises(TypeError, match="CUDA"):
        mid.gather_rows(inp["qkv"], order, inverse, extra)
    with pytest.raises(ValueError, match=r"x must be \[N, W\]"):
        mid.gather_rows(inp["qkv"][0], order, inverse, extra)
    with pytest.raises(TypeError, match="int32"):
        mid.gather_rows(inp["qkv"], order, inverse, extra.long())
    with pytest.raises(ValueError, match="multiple of 4"):
        mid.gather_rows(inp["qkv"][:, :6], order, inverse, extra)
    args = (inp["a"], inverse, extra, inp["x"], inp["wp"], inp["bp"])
    with pytest.raises(TypeError, match="CUDA"):
        mid.proj_residual(*args)
    with pytest.raises(ValueError, match=r"a must be \[T, C\]"):
        mid.proj_residual(inp["a"][0], *args[1:])
    with pytest.raises(ValueError, match="multiple of 4"):
        mid.proj_residual(inp["a"][:, :6], inverse, extra, inp["x"][:, :6], inp["wp"][:6, :6], inp["bp"][:6])
    with pytest.raises(ValueError, match="T >= N"):
        mid.proj_residual(inp["a"][:4], *args[1:])
    with pytest.raises(ValueError, match="T >= N"):
        mid.proj_residual(inp["a"], inverse[:4], *args[2:])
    assert set(mid.stats()) == {"plan_calls", "gather_forward_calls", "gather_backward_calls", "forward_calls", "backward_calls"}


class _FakeCuda:
    """A feature tensor's stand-in that says it is on the GPU: point_mid's checks read its shape only."""
    is_cuda = True

    def __init__(self, shape, dtype=torch.float32):
        self.shape, self.dtype = tuple(shape), dtype

    def dim(self):
        return len(self.shape)


def test_type_and_shape_errors_name_their_rule():
    """(The checks come in the order type, shape, device, so CPU tensors reach the first two.)"""
    inp = R.make_inputs(5, 2, 8, 2)
    order, inverse, extra = inp["order"], inp["inverse"], inp["extra"]
    with pytest.raises(TypeError, match="float32"):
        mid.gather_rows(inp["qkv"].half(), order, inverse, extra)
    with pytest.raises(ValueError, match="x must be"):
        mid.gather_rows(inp["qkv"][:4], order, inverse, extra)              # rows of x against rows of inverse
    with pytest.raises(ValueError, match="extra must be"):
        mid.gather_rows(inp["qkv"], order, inverse, extra[:4])
    args = (inp["a"], inverse, extra, inp["x"], inp["wp"], inp["bp"])
    with pytest.raises(TypeError, match="float32"):
        mid.proj_residual(inp["a"].double(), *args[1:])
    with pytest.raises(ValueError, match="wp must be"):
        mid.proj_residual(*args[:4], inp["wp"][:, :4], inp["bp"])
    with pytest.raises(ValueError, match="bp must be"):
        mid.proj_residual(*args[:5], inp["bp"][:4])
    with pytest.raises(ValueError, match="row_scale must be"):
        mid.proj_residual(*args, inp["r"][:4])
    with pytest.raises(TypeError, match="row_scale must be a float32"):
        mid.proj_residual(*args, inp["r"].double())
    wide = mid.max_channels() + 4
    with pytest.raises(ValueError, match="hold C up to"):
        mid.proj_residual(torch.zeros(7, wide), inverse, extra, torch.zeros(5, wide), torch.zeros(wide, wide), torch.zeros(wide))


@pytest.mark.parametrize("Cn", (4, 32, 48, 128))
def test_torchs_own_float32_run_is_fair_on_these_inputs(Cn):
    """tests/test_front_host.py's bound: torch's float32 formulation on the CPU stays within 2^-19 of the largest element
    of the float64 result in every tensor of the bar, so nothing in the inputs of tests/test_mid_gpu.py (a row scale of
    zeros and 1 / keep, duplicate slots at every row) is beyond float32."""
    for N, D in ((1, 1), (63, 21), (65, 65), (257, 85), (4097, 1300)):
        inp = R.make_inputs(N, D, Cn, 300 + N)
        fig = R.figures(R.run(R.torch_ops, inp, "cpu", torch.float32)[0], R.run(R.torch_ops, inp, "cpu", torch.float64)[0])
        print(Cn, N, D, "worst %.3e" % max(fig.values()))
        assert all(v <= 2.0 ** -19 for v in fig.values()), (Cn, N, D, fig)


def test_the_index_builder_builds_what_it_says():
    for N, D, ident in ((1, 0, True), (1, 1, False), (65, 0, False), (65, 21, False), (257, 257, False)):
        order, inverse, extra = R.make_indices(N, D, 9 + N + D, ident)
        assert order.shape == (N + D,) and inverse.shape == extra.shape == (N,)
        assert sorted(order.tolist()) == sorted(list(range(N)) + order[extra[extra >= 0].long()].tolist())
        assert int((extra >= 0).sum()) == D and torch.equal(torch.from_numpy(R.extra_numpy(order, inverse)), extra)
        assert torch.bincount(order, minlength=N).max() <= 2
        if ident and D == 0:
            assert torch.equal(order, torch.arange(N))
        if D and N > 2:
            dup = extra[extra >= 0]
            assert int(dup.min()) < N                                       # interleaved: not all at the end


# ---- point_mid on a stand-in models.pt_v3 ---------------------------------------------------------------------------------
MINE = "the module's own method"


def _stand_in():
    """What the installs need of models/pt_v3.py, written for this test: a Block that holds its sub-modules under
    upstream's names and a spconv namespace that knows its convolution.  The Block's own forward returns a marker."""
    class Seq(torch.nn.Sequential):
        pass

    class Conv(torch.nn.Module):
        pass

    class DropPath(torch.nn.Module):
        def __init__(self, p):
            super().__init__()
            self.drop_prob, self.scale_by_keep = p, True

    class MLP(torch.nn.Module):
        def __init__(self, c):
            super().__init__()
            self.fc1, self.act, self.fc2 = torch.nn.Linear(c, 4 * c), torch.nn.GELU(), torch.nn.Linear(4 * c, c)

    class Attn(torch.nn.Module):
        def __init__(self, c, proj_bias=True, proj_out=None, proj_drop=0.0, proj=True):
            super().__init__()
            self.channels, self.num_heads, self.enable_flash, self.enable_rpe = c, max(c // 16, 1), False, False
            self.attn_drop, self.proj_drop = torch.nn.Dropout(0.0), torch.nn.Dropout(proj_drop)
            self.qkv = torch.nn.Linear(c, 3 * c)
            self.proj = torch.nn.Linear(c, c if proj_out is None else proj_out, bias=proj_bias) if proj else torch.nn.Identity()

    class Block(torch.nn.Module):
        def __init__(self, c=16, attn=None, drop_path=None):
            super().__init__()
            self.pre_norm = True
            self.cpe = Seq(Conv(), torch.nn.Linear(c, c), torch.nn.LayerNorm(c))
            self.norm1, self.attn = Seq(torch.nn.LayerNorm(c)), attn if attn is not None else Attn(c)
            self.norm2, self.mlp = Seq(torch.nn.LayerNorm(c)), Seq(MLP(c))
            self.drop_path = Seq(torch.nn.Identity() if drop_path is None else drop_path)

        def forward(self, point):
            return MINE

    spconv = types.SimpleNamespace(modules=types.SimpleNamespace(is_spconv_module=lambda m: isinstance(m, Conv)))
    return types.SimpleNamespace(Block=Block, Conv=Conv, Attn=Attn, DropPath=DropPath, spconv=spconv)


def _marks(S):
    return sorted(n for n in vars(S) if n.startswith("_gaussiancity_amd"))


def test_install_installs_point_front_first_and_uninstall_removes_only_the_marker():
    S = _stand_in()
    own = S.Block.forward
    point_mid.uninstall(S)                          # nothing installed: nothing happens
    assert S.Block.forward is own and not _marks(S)
    point_mid.install(S)
    bound = S.Block.forward
    st = point_block.state(S)
    assert bound is not own and st.bound is bound and st.original is own and st.mid is True
    assert st.front == front.max_channels() and st.ffn is None
    point_mid.install(S)                            # idempotent
    assert S.Block.forward is bound
    point_mid.uninstall(S)
    assert S.Block.forward is bound and point_block.state(S).mid is False   # point_front stays
    assert point_block.state(S).front == front.max_channels()
    point_front.uninstall(S)
    assert S.Block.forward is own and not _marks(S)


def test_install_leaves_a_point_front_binding_and_its_cap_as_they_are():
    S = _stand_in()
    own = S.Block.forward
    point_front.install(S, max_channels=64)
    bound = S.Block.forward
    point_mid.install(S)
    assert S.Block.forward is bound and point_block.state(S).front == 64 and point_block.state(S).mid is True
    point_front.uninstall(S)                        # the other order of leaving: the middle alone binds nothing
    st = point_block.state(S)
    assert S.Block.forward is own and len(_marks(S)) == 1
    assert (st.original, st.bound, st.front, st.mid, st.ffn) == (None, None, None, True, None)
    point_mid.uninstall(S)
    assert not _marks(S)


@pytest.mark.parametrize("install_order", ("ffn, mid", "mid, ffn", "front, ffn, mid", "ffn, front, mid"))
def test_point_mid_composes_with_point_ffn_and_point_front_in_either_order(install_order):
    S = _stand_in()
    own = S.Block.forward
    mods = {"ffn": point_ffn, "front": point_front, "mid": point_mid}
    for name in install_order.split(", "):
        mods[name].install(S)
    before = S.Block.forward
    for name in install_order.split(", "):          # idempotent while all are bound
        mods[name].install(S)
        assert S.Block.forward is before
    for m in mods.values():
        m.reset_stats()
    assert S.Block()(types.SimpleNamespace(feat=torch.randn(5, 16))) == MINE    # CPU features: through all to the module
    assert point_front.stats()["original_calls"] == 1 and point_ffn.stats()["original_calls"] == 1
    assert point_mid.stats() == {"fused_calls": 0, "original_calls": 0}         # never asked: point_front turned it away
    point_mid.uninstall(S)
    assert S.Block.forward is before
    point_ffn.uninstall(S)
    point_front.uninstall(S)
    assert S.Block.forward is own and not _marks(S)


def test_what_the_middle_does_not_compute_is_handed_back_and_counted():
    S = _stand_in()
    point = lambda c=16: types.SimpleNamespace(feat=_FakeCuda((5, c)))  # noqa: E731
    assert point_mid.accepts(S.Block(), point(), S) is None                     # not on: nothing is asked or counted
    point_mid.install(S)
    try:
        point_mid.reset_stats()
        cases = {
            "proj without bias": S.Block(attn=S.Attn(16, proj_bias=False)),
            "proj of another width": S.Block(attn=S.Attn(16, proj_out=32)),
            "no Linear as proj": S.Block(attn=S.Attn(16, proj=False)),
            "proj_drop active": S.Block(attn=S.Attn(16, proj_drop=0.1)).train(),
            "a drop_path that is no DropPath": S.Block(drop_path=torch.nn.Dropout(0.1)),
        }
        for why, block in cases.items():
            assert point_mid.accepts(block, point(), S) is None, why
        assert point_mid.stats() == {"fused_calls": 0, "original_calls": len(cases)}
        wide = mid.max_channels() + 16
        assert point_mid._parts(S.Block(c=wide), point(wide)) is None           # point_front's cap is the same: never asked
        accepted = {
            "the plain Block": S.Block(),
            "the cap": S.Block(c=128),
            "proj_drop inactive in eval": S.Block(attn=S.Attn(16, proj_drop=0.1)).eval(),
            "DropPath": S.Block(drop_path=S.DropPath(0.3)),
        }
        for why, block in accepted.items():
            c = block.attn.channels
            parts = point_mid.accepts(block, point(c), S)
            assert parts is not None and parts[0] is block.attn.proj, why
        assert point_mid.accepts(accepted["DropPath"], point(), S)[1].drop_prob == 0.3
        assert point_mid.stats()["original_calls"] == len(cases)
    finally:
        point_mid.uninstall(S)
        point_front.uninstall(S)
