"""The Block-front operator of libgcm_hip.so and its two Python layers without a GPU (not gpu): the four gcm_front_* names
are in the header, the binding table and the library's dynamic symbols, the capability query answers at least 128, every
argument error of the header comes back as GCM_ERR_INVALID_ARGUMENT with a message before a device is touched, the workspace
query is monotone and agrees with the transcribed plan of tests/front_plans.py, whose large cases reach the branches they
name; front.conv_tail_norm_qkv refuses what the library does not run; point_front.install / uninstall rebind and restore
Block.forward of a stand-in models.pt_v3, alone and with point_ffn in both orders, and the method bound at install runs
(and is counted) for everything the operator does not compute."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest
import torch

import front_plans as P
import front_ref as R
from gaussiancity_amd import _native_m as M
from gaussiancity_amd import front, point_block, point_ffn, point_front

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1  # GCM_ERR_INVALID_ARGUMENT
NAMES = {"gcm_front_max_channels", "gcm_front_forward", "gcm_front_backward_workspace_bytes", "gcm_front_backward"}


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
    assert M.lib().gcm_front_max_channels() >= 128 and front.max_channels() == M.lib().gcm_front_max_channels()


@pytest.fixture()
def mem():
    """(the library, a 256-byte aligned address of host memory that no call below reaches the point of using)."""
    buf = (C.c_float * 1024)()
    return M.lib(), buf, (C.addressof(buf) + 255) // 256 * 256


FWD_PTRS = ("x", "s", "wc", "bc", "lnc_w", "lnc_b", "ln1_w", "ln1_b", "wq", "bq", "feat", "qkv")
BWD_IN = ("s", "feat", "t", "mean_c", "rstd_c", "mean_1", "rstd_1", "dfeat", "dqkv", "wc", "lnc_w", "ln1_w", "ln1_b", "wq")
BWD_OUT = ("dx", "ds", "dwc", "dbc", "dlnc_w", "dlnc_b", "dln1_w", "dln1_b", "dwq", "dbq")


def _forward(lib, p, xs=8, ss=8, fs=8, qs=24, N=4, Cn=8, O=24, eps_c=1e-5, eps_1=1e-5, t=None, stats=(None,) * 4, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    return lib.gcm_front_forward(g("x"), xs, g("s"), ss, g("wc"), g("bc"), g("lnc_w"), g("lnc_b"), eps_c, g("ln1_w"),
                                 g("ln1_b"), eps_1, g("wq"), g("bq"), N, Cn, O, g("feat"), fs, g("qkv"), qs, t, *stats, None)


def _backward(lib, p, ss=8, fs=8, dfs=8, dqs=24, dxs=8, dss=8, N=4, Cn=8, O=24, work="p", bytes_=None, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    need = lib.gcm_front_backward_workspace_bytes(N, Cn, O) if bytes_ is None else bytes_
    return lib.gcm_front_backward(g("s"), ss, g("feat"), fs, g("t"), g("mean_c"), g("rstd_c"), g("mean_1"), g("rstd_1"),
                                  g("dfeat"), dfs, g("dqkv"), dqs, g("wc"), g("lnc_w"), g("ln1_w"), g("ln1_b"), g("wq"), N, Cn,
                                  O, g("dx"), dxs, g("ds"), dss, g("dwc"), g("dbc"), g("dlnc_w"), g("dlnc_b"), g("dln1_w"),
                                  g("dln1_b"), g("dwq"), g("dbq"), p if work == "p" else work, need, None)


def _refused(lib, rc, text):
    assert rc == INVALID, rc
    msg = lib.gcm_last_error()
    assert msg and text in msg, msg
    with pytest.raises(RuntimeError, match="gcm_status -1"):
        M.check(rc, "call")


def test_forward_argument_errors_come_back_before_a_device_is_touched(mem):
    lib, _, p = mem
    limit = lib.gcm_front_max_channels()
    for bad in (6, 0, -4):
        _refused(lib, _forward(lib, p, Cn=bad), b"C must be")
        _refused(lib, _forward(lib, p, O=bad), b"O must be")
    wide = limit + 4
    _refused(lib, _forward(lib, p, Cn=wide, xs=wide, ss=wide, fs=wide, O=3 * wide, qs=3 * wide), b"C above")
    _refused(lib, _forward(lib, p, O=3 * limit + 4, qs=3 * limit + 4), b"O above")
    for stride in ("xs", "ss", "fs", "qs"):
        for bad in (6, 0, -8, 4):  # not a multiple of 4, not positive, shorter than the row
            _refused(lib, _forward(lib, p, **{stride: bad}), b"strides")
    for name in FWD_PTRS:
        _refused(lib, _forward(lib, p, **{name: p + 4}), b"16-byte")
    _refused(lib, _forward(lib, p, t=p + 4, stats=(p,) * 4), b"16-byte")
    _refused(lib, _forward(lib, p, N=-1), b"N out of range")
    _refused(lib, _forward(lib, p, eps_c=-1.0), b"eps")
    _refused(lib, _forward(lib, p, eps_1=-1.0), b"eps")
    for name in FWD_PTRS:
        _refused(lib, _forward(lib, p, **{name: None}), b"null")
    _refused(lib, _forward(lib, p, t=p), b"all or none")                          # t without the statistics
    _refused(lib, _forward(lib, p, stats=(p,) * 4), b"all or none")               # the statistics without t
    for k in range(4):                                                             # three of the four
        _refused(lib, _forward(lib, p, t=p, stats=tuple(None if j == k else p for j in range(4))), b"all or none")
    assert _forward(lib, p, N=0) == 0  # an empty problem is fine and queues nothing


def test_backward_argument_errors_and_a_short_null_or_misaligned_workspace(mem):
    lib, _, p = mem
    limit = lib.gcm_front_max_channels()
    _refused(lib, _backward(lib, p, Cn=10, bytes_=1 << 20), b"C must be")
    _refused(lib, _backward(lib, p, O=2, bytes_=1 << 20), b"O must be")
    wide = limit + 4
    _refused(lib, _backward(lib, p, Cn=wide, ss=wide, fs=wide, dfs=wide, dxs=wide, dss=wide, bytes_=1 << 30), b"C above")
    _refused(lib, _backward(lib, p, O=3 * limit + 4, dqs=3 * limit + 4, bytes_=1 << 30), b"O above")
    for stride in ("ss", "fs", "dfs", "dqs", "dxs", "dss"):
        for bad in (10, 4, 0):
            _refused(lib, _backward(lib, p, **{stride: bad}), b"strides")
    for name in BWD_IN + BWD_OUT:
        if name not in ("mean_c", "rstd_c", "mean_1", "rstd_1"):               # the statistics are 4-byte aligned
            _refused(lib, _backward(lib, p, **{name: p + 8}), b"16-byte")
    need = lib.gcm_front_backward_workspace_bytes(4, 8, 24)
    assert need > 0
    _refused(lib, _backward(lib, p, bytes_=need - 1), b"workspace smaller")
    _refused(lib, _backward(lib, p, work=None), b"workspace smaller")
    _refused(lib, _backward(lib, p, work=p + 16), b"256-byte")
    for name in BWD_IN:                                                         # both gradients are required too
        _refused(lib, _backward(lib, p, **{name: None}), b"null")
    _refused(lib, _backward(lib, p, N=-1, bytes_=1 << 20), b"N out of range")


def test_workspace_query_is_monotone_in_the_rows_and_refuses_bad_shapes():
    lib = M.lib()
    for Cn, O in ((4, 12), (32, 96), (48, 40), (128, 384)):
        sizes = [lib.gcm_front_backward_workspace_bytes(n, Cn, O) for n in (0, 1, 63, 64, 65, 130, 333, 4096, 4160, 65536, 262144)]
        assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[0] % 256 == 0 and sizes[-1] >= 262144 * Cn * 4, sizes
    assert lib.gcm_front_backward_workspace_bytes(10, 6, 8) == 0 and b"C must be" in lib.gcm_last_error()
    assert lib.gcm_front_backward_workspace_bytes(10, 8, 6) == 0 and b"O must be" in lib.gcm_last_error()
    assert lib.gcm_front_backward_workspace_bytes(10, 132, 384) == 0 and b"C above" in lib.gcm_last_error()
    assert lib.gcm_front_backward_workspace_bytes(10, 128, 388) == 0 and b"O above" in lib.gcm_last_error()
    assert lib.gcm_front_backward_workspace_bytes(-1, 8, 8) == 0 and lib.gcm_last_error()


# ---- the plan ---------------------------------------------------------------------------------------------------------------
WIDTHS = ((4, 12), (32, 96), (48, 40), (128, 384), (36, 108), (68, 204), (100, 300), (128, 4), (128, 8), (64, 192), (4, 384))
NS = (0, 1, 63, 64, 65, 130, 4095, 4096, 4097, 8193, 65536)


def test_the_transcribed_plan_carves_what_the_library_asks_for():
    lib = M.lib()
    for shape in [(N, Cn, O) for (Cn, O) in WIDTHS for N in NS] + list(P.PLAN_CASES):
        p = P.front_plan(*shape)
        assert lib.gcm_front_backward_workspace_bytes(*shape) == p["total"], (shape, p)
        assert all(off % 256 == 0 for off in p["at"].values()) and p["total"] % 256 == 0
        assert (p["groups"] == 0) == (shape[0] <= 4096), shape          # the second fold level starts past 64 tiles
        assert p["launches"] == (4 if shape[0] <= 4096 else 5)          # and the launches do not grow with N otherwise
        assert p["sw"] <= P.MAX_SLICES


def test_the_slices_cover_every_row_once_and_the_groups_every_tile_once():
    for shape in P.PLAN_CASES:
        p = P.front_plan(*shape)
        N, rows = shape[0], 0
        for s in range(p["sw"]):
            p0 = s * p["per"]
            rows += max(min(p0 + p["per"], N) - p0, 0)
        assert rows == N and p["per"] % P.KC == 0, (shape, p)
        tiles = sum(max(min((q + 1) * p["gper"], p["tiles"]) - q * p["gper"], 0) for q in range(p["groups"]))
        assert tiles == p["tiles"] and (p["groups"] - 1) * p["gper"] < p["tiles"], (shape, p)


@pytest.mark.parametrize("shape", sorted(P.PLAN_CASES))
def test_every_plan_case_reaches_the_branch_it_names(shape):
    stated, derived = P.PLAN_CASES[shape], P.facts(shape)
    assert stated and set(stated) <= set(derived)
    wrong = {k: (v, derived[k]) for k, v in stated.items() if derived[k] != v}
    assert not wrong, (shape, wrong)


@pytest.mark.parametrize("name", [n for n, _ in P.BRANCH_FACTS])
def test_every_branch_fact_is_held_by_a_case_and_by_none_of_the_small_shapes(name):
    holds = dict(P.BRANCH_FACTS)[name]
    assert [shape for shape in P.PLAN_CASES if holds(P.facts(shape))], name
    assert not [(Cn, O) for Cn, O in ((4, 12), (32, 96), (48, 40), (128, 384)) if holds(P.facts((257, Cn, O)))
                and name != "a weight-gradient chain longer than kFfnSumRows"], name


# ---- the Python operator ------------------------------------------------------------------------------------------------------
def _cpu_args(Cn=8, O=24, N=4):
    inp = R.make_inputs(N, Cn, O, 1)
    return [inp["x"], inp["s"], inp["wc"], inp["bc"], inp["gc"], inp["bec"], 1e-5, inp["g1"], inp["be1"], 1e-5, inp["wq"], inp["bq"]]


def test_the_operator_refuses_what_the_library_does_not_run():
    args = _cpu_args()
    with pytest.raises(TypeError, match="CUDA"):
        front.conv_tail_norm_qkv(*args)
    with pytest.raises(TypeError, match="float32"):
        front.conv_tail_norm_qkv(args[0].half(), *args[1:])
    with pytest.raises(ValueError, match="multiples of 4"):
        front.conv_tail_norm_qkv(*_cpu_args(Cn=6))
    with pytest.raises(ValueError, match="multiples of 4"):
        front.conv_tail_norm_qkv(*_cpu_args(O=10))
    with pytest.raises(ValueError, match=r"x must be \[N, C\]"):
        front.conv_tail_norm_qkv(args[0][0], *args[1:])
    assert set(front.stats()) == {"forward_calls", "backward_calls"}


@pytest.mark.parametrize("Cn,O", ((4, 12), (32, 96), (48, 40), (128, 384)))
def test_torchs_own_float32_run_handles_the_special_rows(Cn, O):
    """The inputs of test_front_gpu.py's special-rows case are fair: torch's float32 formulation on the CPU stays within
    2^-19 of the largest element of the float64 result in every tensor -- sqrt(384) * 2^-24 = 1.2e-6 is the random-walk
    rounding of the longest sum there, rounded up to a power of two -- so nothing in them (rstd = 1 / sqrt(eps) on the
    constant row, a factor 1e6 between two rows) is beyond float32."""
    for N in (63, 65, 257, 4097):
        inp = R.special_rows(R.make_inputs(N, Cn, O, 300 + N))
        t64 = inp["s"].double() @ inp["wc"].double().T + inp["bc"].double()
        assert float(t64[3].var(unbiased=False)) == 0.0
        fig = R.figures(R.run(R.torch_ops, inp, "cpu", torch.float32), R.run(R.torch_ops, inp, "cpu", torch.float64))
        print(Cn, O, N, "worst %.3e" % max(fig.values()))
        assert all(v <= 2.0 ** -19 for v in fig.values()), (Cn, O, N, fig)


# ---- point_front on a stand-in models.pt_v3 ---------------------------------------------------------------------------------
MINE = "the module's own method"


def _stand_in():
    """What install() needs of models/pt_v3.py, written for this test: a Block that holds its sub-modules under
    upstream's names and a spconv namespace that knows its convolution.  The Block's own forward returns a marker, so a
    test can tell which method ran."""
    class Seq(torch.nn.Sequential):
        pass

    class Conv(torch.nn.Module):
        pass

    class MLP(torch.nn.Module):
        def __init__(self, c):
            super().__init__()
            self.fc1, self.act, self.fc2 = torch.nn.Linear(c, 4 * c), torch.nn.GELU(), torch.nn.Linear(4 * c, c)

    class Attn(torch.nn.Module):
        def __init__(self, c, heads, flash=False, rpe=False, qkv_bias=True, out=None):
            super().__init__()
            self.channels, self.num_heads, self.enable_flash, self.enable_rpe = c, heads, flash, rpe
            self.attn_drop = torch.nn.Dropout(0.0)
            self.qkv = torch.nn.Linear(c, 3 * c if out is None else out, bias=qkv_bias)

    class Block(torch.nn.Module):
        def __init__(self, c=16, pre_norm=True, cpe=None, norm1=None, attn=None):
            super().__init__()
            self.pre_norm = pre_norm
            self.cpe = Seq(*cpe) if cpe is not None else Seq(Conv(), torch.nn.Linear(c, c), torch.nn.LayerNorm(c))
            self.norm1 = Seq(norm1 if norm1 is not None else torch.nn.LayerNorm(c))
            self.attn = attn if attn is not None else Attn(c, c // 16 if c >= 16 else 1)
            self.norm2, self.mlp, self.drop_path = Seq(torch.nn.LayerNorm(c)), Seq(MLP(c)), Seq(torch.nn.Identity())

        def forward(self, point):
            return MINE

    spconv = types.SimpleNamespace(modules=types.SimpleNamespace(is_spconv_module=lambda m: isinstance(m, Conv)))
    return types.SimpleNamespace(Block=Block, Conv=Conv, Attn=Attn, spconv=spconv)


def test_install_and_uninstall_are_idempotent_and_restore_the_method():
    S = _stand_in()
    own = S.Block.forward
    point_front.uninstall(S)  # nothing installed: nothing happens
    assert S.Block.forward is own
    point_front.install(S)
    bound = S.Block.forward
    assert bound is not own
    point_front.install(S)
    st = point_block.state(S)
    assert S.Block.forward is bound and st.bound is bound and st.original is own and st.front == front.max_channels()
    point_front.uninstall(S)
    assert S.Block.forward is own and not [n for n in vars(S) if n.startswith("_gaussiancity_amd")]
    point_front.uninstall(S)
    assert S.Block.forward is own
    with pytest.raises(ValueError, match="max_channels"):
        point_front.install(S, max_channels=-4)
    assert S.Block.forward is own


@pytest.mark.parametrize("install_order", ("ffn, front", "front, ffn"))
@pytest.mark.parametrize("uninstall_order", ("ffn, front", "front, ffn"))
def test_point_ffn_and_point_front_compose_in_either_order(install_order, uninstall_order):
    S = _stand_in()
    own = S.Block.forward
    mods = {"ffn": point_ffn, "front": point_front}
    for name in install_order.split(", "):
        mods[name].install(S)
    assert S.Block.forward is not own
    for name in install_order.split(", "):      # idempotent while both are bound
        before = S.Block.forward
        mods[name].install(S)
        assert S.Block.forward is before
    point_front.reset_stats()
    point_ffn.reset_stats()
    assert S.Block()(types.SimpleNamespace(feat=torch.randn(5, 16))) == MINE    # CPU features: through both to the module
    assert point_front.stats()["original_calls"] == 1 and point_ffn.stats()["original_calls"] == 1
    first, second = uninstall_order.split(", ")
    mods[first].uninstall(S)
    assert S.Block()(types.SimpleNamespace(feat=torch.randn(5, 16))) == MINE    # whatever is bound now still ends there
    mods[second].uninstall(S)
    assert S.Block.forward is own and not [n for n in vars(S) if n.startswith("_gaussiancity_amd")]


def test_point_ffns_uninstall_leaves_point_front_running(monkeypatch):
    S = _stand_in()
    own = S.Block.forward
    point_ffn.install(S)
    point_front.install(S)
    first = S.Block.forward
    point_ffn.uninstall(S)                      # the front stays on, under the same method
    st = point_block.state(S)
    assert S.Block.forward is first and st.bound is first and st.original is own and st.ffn is None and st.front is not None

    class Reached(Exception):
        pass

    def stub(*args):
        raise Reached
    monkeypatch.setattr(front, "conv_tail_norm_qkv", stub)
    block, point = S.Block(), _point()
    block.cpe[0].forward = lambda sparse: types.SimpleNamespace(features=None)
    point.sparse_conv_feat = None
    with pytest.raises(Reached):                # a Block the front accepts reaches the fused front
        block(point)
    point_front.uninstall(S)
    assert S.Block.forward is own and point_block.state(S) is None
    assert not [n for n in vars(S) if n.startswith("_gaussiancity_amd")]


class _FakeCuda:
    """A feature tensor's stand-in that says it is on the GPU: the checks that come after the device are reached here."""
    is_cuda = True

    def __init__(self, n, c, dtype=torch.float32):
        self.shape, self.dtype = (n, c), dtype

    def dim(self):
        return 2


def _point(c=16, dtype=torch.float32):
    return types.SimpleNamespace(feat=_FakeCuda(5, c, dtype))


def test_what_the_operator_does_not_compute_reaches_the_method_bound_at_install_and_is_counted():
    S = _stand_in()
    point_front.install(S)
    try:
        point_front.reset_stats()
        lin, ln = (lambda c=16, **k: torch.nn.Linear(c, c, **k)), (lambda c=16, **k: torch.nn.LayerNorm(c, **k))
        cases = {
            "CPU tensors": (S.Block(), types.SimpleNamespace(feat=torch.randn(5, 16))),
            "post-norm": (S.Block(pre_norm=False), _point()),
            "two modules in cpe": (S.Block(cpe=(S.Conv(), lin())), _point()),
            "four modules in cpe": (S.Block(cpe=(S.Conv(), lin(), ln(), torch.nn.Identity())), _point()),
            "no spconv module first": (S.Block(cpe=(torch.nn.Identity(), lin(), ln())), _point()),
            "a Linear without bias": (S.Block(cpe=(S.Conv(), lin(bias=False), ln())), _point()),
            "a Linear that changes the width": (S.Block(cpe=(S.Conv(), torch.nn.Linear(16, 32), ln(32))), _point()),
            "no Linear second": (S.Block(cpe=(S.Conv(), torch.nn.Identity(), ln())), _point()),
            "a BatchNorm third": (S.Block(cpe=(S.Conv(), lin(), torch.nn.BatchNorm1d(16))), _point()),
            "a LayerNorm without affine": (S.Block(cpe=(S.Conv(), lin(), ln(elementwise_affine=False))), _point()),
            "norm1 a BatchNorm": (S.Block(norm1=torch.nn.BatchNorm1d(16)), _point()),
            "norm1 without bias": (S.Block(norm1=ln(bias=False)), _point()),
            "qkv without bias": (S.Block(attn=S.Attn(16, 1, qkv_bias=False)), _point()),
            "qkv of another input width": (S.Block(c=32), _point(16)),
            "the flash branch": (S.Block(attn=S.Attn(16, 1, flash=True)), _point()),
            "relative position encoding": (S.Block(attn=S.Attn(16, 1, rpe=True)), _point()),
            "a head width the attention does not run": (S.Block(attn=S.Attn(16, 4)), _point()),
            "float16 features": (S.Block(), _point(dtype=torch.float16)),
            "C no multiple of 4": (S.Block(c=18, attn=S.Attn(18, 1)), _point(18)),
            "O no multiple of 4": (S.Block(attn=S.Attn(16, 1, out=50)), _point()),
            "C above the limit": (S.Block(c=front.max_channels() + 16), _point(front.max_channels() + 16)),
        }
        for why, (block, point) in cases.items():
            assert block(point) == MINE, why
        torch.set_autocast_enabled(True)  # (the context manager switches itself off where no GPU is visible)
        try:
            assert S.Block()(_point()) == MINE
        finally:
            torch.set_autocast_enabled(False)
        assert point_front.stats() == {"fused_calls": 0, "original_calls": len(cases) + 1}
        # the stand-in that says it is on the GPU passes every check when nothing is in the way: the cases above were
        # turned away by what they name, not by the stand-in
        assert point_front._parts(S.Block(), _point(), S) is not None
        assert point_front._parts(S.Block(c=128), _point(128), S) is not None
        point_front.reset_stats()
        assert point_front.stats() == {"fused_calls": 0, "original_calls": 0}
    finally:
        point_front.uninstall(S)


def test_max_channels_caps_the_width_that_takes_the_fused_front():
    S = _stand_in()
    point_front.install(S, max_channels=64)
    try:
        point_front.reset_stats()
        assert point_front._parts(S.Block(c=64), _point(64), S) is not None
        assert point_front._parts(S.Block(c=128), _point(128), S) is None
        assert S.Block(c=128)(_point(128)) == MINE and point_front.stats()["original_calls"] == 1
        bound = S.Block.forward
        point_front.install(S)                    # the default again, the binding stays
        assert S.Block.forward is bound and point_front._parts(S.Block(c=128), _point(128), S) is not None
        point_front.install(S, max_channels=10 ** 6)   # never beyond the library's limit
        wide = front.max_channels() + 16
        assert point_front._parts(S.Block(c=wide), _point(wide), S) is None
    finally:
        point_front.uninstall(S)
