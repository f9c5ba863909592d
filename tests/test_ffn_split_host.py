"""The split feed-forward entry points of libgcm_hip.so and their two Python layers without a GPU (not gpu): the five
gcm_ffn_split_* names are in the header, the binding table and the library's dynamic symbols; the plan query equals its
transcription (tests/ffn_split_plans.py) over a grid of shapes and the workspace sizes follow from it; every argument error
comes back as GCM_ERR_INVALID_ARGUMENT with its rule named before a device is touched; and point_ffn.install's keywords route
the Blocks of a stand-in models.pt_v3 -- alone and composed with point_front -- as its docstring says."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest
import torch

import ffn_split_plans as plans
from gaussiancity_amd import _native_m as M
from gaussiancity_amd import ffn, point_ffn, point_front
from test_ffn_host import _FakeCuda, _refused, _stand_in
from test_front_host import _stand_in as _front_stand_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gcm_ffn_split_max_channels", "gcm_ffn_split_plan", "gcm_ffn_split_workspace_bytes", "gcm_ffn_split_forward",
         "gcm_ffn_split_backward"}
MINE = "the module's own method"


def test_the_five_names_are_in_the_header_the_binding_and_the_library():
    lib = M.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gcm.h")).read(), flags=re.S)
    assert NAMES <= set(re.findall(r"\b(gcm_[a-z_]+)\s*\(", header))
    assert NAMES <= set(M.EXPORTED_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", M.LIB_PATH]).decode()
    assert NAMES <= set(re.findall(r" T (gcm_[a-z_]+)", out))
    assert not [name for name in NAMES if getattr(lib, name).argtypes is None]
    assert lib.gcm_abi_version() == 1
    assert lib.gcm_ffn_split_max_channels() == 512 == ffn.split_max_channels()
    assert lib.gcm_ffn_max_channels() == ffn.max_channels() < ffn.split_max_channels()   # the old limit did not move


def _query(lib, N, Cn, Hd):
    plan, fwd, bwd = (C.c_int64 * 8)(), C.c_size_t(), C.c_size_t()
    assert lib.gcm_ffn_split_plan(N, Cn, Hd, plan) == 0, lib.gcm_last_error()
    assert lib.gcm_ffn_split_workspace_bytes(N, Cn, Hd, C.byref(fwd), C.byref(bwd)) == 0, lib.gcm_last_error()
    return list(plan), fwd.value, bwd.value


def test_the_plan_query_equals_its_transcription_and_the_workspaces_follow_from_it():
    lib = M.lib()
    limit = _query(lib, 1, 4, 4)[0][6]
    assert limit >= 1
    modes = set()
    for Cn, Hd in ((4, 4), (32, 128), (48, 40), (128, 512), (132, 528), (132, 72), (256, 1024), (388, 200), (512, 2048)):
        edge = plans.first_rows_mode_n(Hd, limit)        # both sides of the mode limit
        last = {}
        for N in sorted({0, 1, 63, 64, 65, 257, 4096, 4097, edge - 64, edge - 1, edge, edge + 64, 4 * edge}):
            want = plans.split_plan(N, Cn, Hd, limit)
            plan, fwd, bwd = _query(lib, N, Cn, Hd)
            assert plan == plans.as_query(want), (N, Cn, Hd, plan, want)
            assert (fwd, bwd) == (want["forward"], want["backward"]), (N, Cn, Hd)
            assert plan[0] == (1 if plan[1] * plan[2] <= limit else 0) and plan[3] == (plan[2] if plan[0] else 1)
            assert plan[2] == -(-Hd // 64)
            assert fwd % 256 == 0 and bwd % 256 == 0 and fwd >= max(256, plan[3] * N * Cn * 4)
            if Cn <= ffn.max_channels():                  # the one-launch backward's pieces and the dxn records besides
                assert bwd >= lib.gcm_ffn_backward_workspace_bytes(N, Cn, Hd) + plan[3] * N * Cn * 4
            assert bwd >= (N * Hd + plan[3] * N * Cn + plan[1] * 2 * Cn + plan[4] * (2 * Cn * Hd + Hd + Cn)) * 4
            if plan[0] in last:                           # monotone in N within a mode
                assert fwd >= last[plan[0]][0] and bwd >= last[plan[0]][1], (N, Cn, Hd)
            last[plan[0]] = (fwd, bwd)
            modes.add(plan[0])
        assert _query(lib, edge, Cn, Hd)[0][0] == 0 and _query(lib, edge - 1, Cn, Hd)[0][0] == 1
    assert modes == {0, 1}
    assert ffn.split_plan(257, 132, 528) == {"mode": "split", "tiles": 5, "chunks": 9, "records": 9, "weight_slices": 5,
                                             "ln_groups": 0, "limit": limit}
    plan = (C.c_int64 * 8)()
    for shape, text in (((10, 6, 8), b"C must be"), ((10, 8, 6), b"Hd must be"), ((10, 516, 512), b"C above"),
                        ((10, 512, 2052), b"Hd above"), ((-1, 8, 8), b"N out of range")):
        _refused(lib, lib.gcm_ffn_split_plan(*shape, plan), text)
        _refused(lib, lib.gcm_ffn_split_workspace_bytes(*shape, None, None), text)
    _refused(lib, lib.gcm_ffn_split_plan(10, 8, 8, None), b"null plan")


@pytest.fixture()
def mem():
    """(the library, a 256-byte aligned address of host memory that no call below reaches the point of using)."""
    buf = (C.c_float * 1024)()
    return M.lib(), buf, (C.addressof(buf) + 255) // 256 * 256


def _forward(lib, p, xs=8, ys=8, N=4, Cn=8, Hd=16, eps=1e-5, a=None, mean=None, rstd=None, work="p", bytes_=None, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    need = bytes_
    if need is None:
        fwd = C.c_size_t(1 << 20)
        lib.gcm_ffn_split_workspace_bytes(N, Cn, Hd, C.byref(fwd), None)
        need = fwd.value
    return lib.gcm_ffn_split_forward(g("x"), xs, g("ln_w"), g("ln_b"), eps, g("w1"), g("b1"), g("w2"), g("b2"), None, N, Cn, Hd,
                                     g("y"), ys, mean, rstd, a, p if work == "p" else work, need, None)


def _backward(lib, p, xs=8, dys=8, dxs=8, N=4, Cn=8, Hd=16, work="p", bytes_=None, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    need = bytes_
    if need is None:
        bwd = C.c_size_t(1 << 20)
        lib.gcm_ffn_split_workspace_bytes(N, Cn, Hd, None, C.byref(bwd))
        need = bwd.value
    return lib.gcm_ffn_split_backward(g("x"), xs, p, p, g("a"), g("dy"), dys, None, g("ln_w"), g("ln_b"), g("w1"), g("w2"), N, Cn,
                                      Hd, g("dx"), dxs, g("dln_w"), g("dln_b"), g("dw1"), g("db1"), g("dw2"), g("db2"),
                                      p if work == "p" else work, need, None)


def test_forward_argument_errors_come_back_before_a_device_is_touched(mem):
    lib, _, p = mem
    for bad in (6, 0, -4):
        _refused(lib, _forward(lib, p, Cn=bad), b"C must be")
        _refused(lib, _forward(lib, p, Hd=bad), b"Hd must be")
    _refused(lib, _forward(lib, p, Cn=516, xs=516, ys=516), b"C above gcm_ffn_split_max_channels")
    _refused(lib, _forward(lib, p, Hd=2052), b"Hd above")
    for stride in ("xs", "ys"):
        for bad in (6, 0, -8, 4):  # not a multiple of 4, not positive, shorter than the row
            _refused(lib, _forward(lib, p, **{stride: bad}), b"strides")
    _refused(lib, _forward(lib, p, Cn=512, Hd=2048, xs=508, ys=512), b"strides")
    for name in ("x", "ln_w", "ln_b", "w1", "b1", "w2", "b2", "y"):
        _refused(lib, _forward(lib, p, **{name: p + 4}), b"16-byte")
    _refused(lib, _forward(lib, p, a=p + 4, mean=p, rstd=p), b"16-byte")
    _refused(lib, _forward(lib, p, N=-1), b"N out of range")
    _refused(lib, _forward(lib, p, eps=-1.0), b"eps")
    fwd = C.c_size_t()
    assert lib.gcm_ffn_split_workspace_bytes(4, 8, 16, C.byref(fwd), None) == 0 and fwd.value >= 256
    _refused(lib, _forward(lib, p, bytes_=fwd.value - 1), b"workspace smaller")
    _refused(lib, _forward(lib, p, work=None), b"workspace smaller")
    _refused(lib, _forward(lib, p, work=p + 16), b"256-byte")
    _refused(lib, _forward(lib, p, x=None), b"null")
    _refused(lib, _forward(lib, p, a=p), b"mean and rstd")
    _refused(lib, _forward(lib, p, mean=p), b"mean and rstd")
    assert _forward(lib, p, N=0) == 0  # an empty problem is fine and queues nothing


def test_backward_argument_errors_and_a_short_null_or_misaligned_workspace(mem):
    lib, _, p = mem
    _refused(lib, _backward(lib, p, Cn=10), b"C must be")
    _refused(lib, _backward(lib, p, Hd=2), b"Hd must be")
    _refused(lib, _backward(lib, p, Cn=516, xs=516, dys=516, dxs=516), b"C above gcm_ffn_split_max_channels")
    _refused(lib, _backward(lib, p, Hd=2052), b"Hd above")
    for stride in ("xs", "dys", "dxs"):
        for bad in (10, 4, 0):
            _refused(lib, _backward(lib, p, **{stride: bad}), b"strides")
    for name in ("x", "a", "dy", "ln_w", "ln_b", "w1", "w2", "dx", "dln_w", "dln_b", "dw1", "db1", "dw2", "db2"):
        _refused(lib, _backward(lib, p, **{name: p + 8}), b"16-byte")
    bwd = C.c_size_t()
    assert lib.gcm_ffn_split_workspace_bytes(4, 8, 16, None, C.byref(bwd)) == 0 and bwd.value > 0
    _refused(lib, _backward(lib, p, bytes_=bwd.value - 1), b"workspace smaller")
    _refused(lib, _backward(lib, p, work=None), b"workspace smaller")
    _refused(lib, _backward(lib, p, work=p + 16), b"256-byte")
    _refused(lib, _backward(lib, p, x=None), b"null")


def test_the_operator_names_the_split_limit_and_keeps_the_old_one_by_default():
    assert set(ffn.stats()) == {"forward_calls", "backward_calls"} == set(ffn.split_stats())
    args = [torch.randn(4, 8), torch.ones(8), torch.zeros(8), 1e-5, torch.randn(16, 8), torch.zeros(16), torch.randn(8, 16),
            torch.zeros(8)]
    with pytest.raises(TypeError, match="CUDA"):
        ffn.layernorm_mlp_residual(*args, split=True)


# ---- point_ffn's keywords on a stand-in models.pt_v3 ------------------------------------------------------------------------
class _Pass(torch.nn.Module):
    """Upstream's front and middle modules for a point that holds no tensor: the point goes through."""
    def forward(self, point):
        return point


def _point(n, c):
    return types.SimpleNamespace(feat=_FakeCuda(n, c))


def _block(P, c, hidden=None):
    b = P.Block(c=c)
    if hidden is not None:
        b.mlp[0].fc1, b.mlp[0].fc2 = torch.nn.Linear(c, hidden), torch.nn.Linear(hidden, c)
    return b


def test_the_default_install_turns_a_wide_block_away_and_max_channels_admits_it():
    P = _stand_in()
    point_ffn.install(P)
    try:
        point_ffn.reset_stats()
        assert P.Block(c=256)(_point(5, 256)) == MINE
        assert point_ffn.stats() == {"fused_calls": 0, "original_calls": 1} and point_ffn.split_stats() == {"fused_calls": 0}
        assert point_ffn._parts(P.Block(c=256), _point(5, 256), P) is None
        assert point_ffn._parts(P.Block(c=8), _point(5, 8), P) is not None and not point_ffn.takes_split(P, 8)
        point_ffn.install(P, max_channels=512)            # the keywords of a second install are taken over
        for c in (256, 512):
            assert point_ffn._parts(P.Block(c=c), _point(5, c), P) is not None and point_ffn.takes_split(P, c)
            assert point_ffn._parts(P.Block(c=c), _point(5, c)) is None      # without the module: the old limit
        assert point_ffn._parts(P.Block(c=516), _point(5, 516), P) is None
        assert P.Block(c=516)(_point(5, 516)) == MINE
        assert point_ffn._parts(_block(P, 512, 2052), _point(5, 512), P) is None
        assert point_ffn._parts(_block(P, 128, 1024), _point(5, 128), P) is None   # narrow: the one-launch kernels' hidden limit
        assert point_ffn._parts(P.Block(c=8), _point(5, 8), P) is not None and not point_ffn.takes_split(P, 8)
        point_ffn.install(P, max_channels=256)
        assert point_ffn._parts(P.Block(c=256), _point(5, 256), P) is not None
        assert point_ffn._parts(P.Block(c=260), _point(5, 260), P) is None
        point_ffn.install(P, split=True)
        assert point_ffn.takes_split(P, 8) and point_ffn._parts(P.Block(c=8), _point(5, 8), P) is not None
        assert point_ffn._parts(_block(P, 128, 1024), _point(5, 128), P) is not None
        assert point_ffn._parts(P.Block(c=256), _point(5, 256), P) is None       # split alone does not widen
    finally:
        point_ffn.uninstall(P)
    assert not [n for n in vars(P) if n.startswith("_gaussiancity_amd_point_ffn")]


def test_split_routes_a_narrow_block_to_the_split_path(monkeypatch):
    """The rebound method reaches ffn.layernorm_mlp_residual with split=True and counts it."""
    P = _stand_in()
    seen = []

    def operator(feat, *args, split=False):
        seen.append(split)
        return feat

    monkeypatch.setattr(ffn, "layernorm_mlp_residual", operator)
    conv = types.SimpleNamespace(replace_feature=lambda f: f)
    for kwargs, c, want in (({"split": True}, 8, True), ({}, 8, False), ({"max_channels": 512}, 256, True),
                            ({"max_channels": 512}, 128, False), ({"max_channels": 512, "split": True}, 128, True)):
        point_ffn.install(P, **kwargs)
        try:
            point_ffn.reset_stats()
            block = P.Block(c=c)
            point = types.SimpleNamespace(feat=_FakeCuda(5, c), sparse_conv_feat=conv)
            point.feat.__class__ = type("Feat", (_FakeCuda,), {"__add__": lambda a, b: a, "__radd__": lambda a, b: a})
            assert block(point) is point and seen[-1] is want, (kwargs, c)
            assert point_ffn.stats() == {"fused_calls": 1, "original_calls": 0}
            assert point_ffn.split_stats() == {"fused_calls": int(want)}
        finally:
            point_ffn.uninstall(P)


def test_bad_keyword_values_raise():
    P = _stand_in()
    own = P.Block.forward
    for kwargs in ({"max_channels": -1}, {"max_channels": 2.0}, {"max_channels": "512"}, {"max_channels": True},
                   {"max_channels": 516}, {"split": 1}, {"split": None}, {"split": "yes"}):
        with pytest.raises(ValueError):
            point_ffn.install(P, **kwargs)
        assert P.Block.forward is own and not [n for n in vars(P) if n.startswith("_gaussiancity_amd")], kwargs


@pytest.mark.parametrize("front_first", (True, False))
@pytest.mark.parametrize("ffn_leaves_first", (True, False))
def test_with_point_front_installed_a_wide_block_reaches_point_ffns_tail_and_both_uninstall_orders_restore(
        monkeypatch, front_first, ffn_leaves_first):
    P = _front_stand_in()                                 # a Block whose front point_front accepts up to its own limit
    own = P.Block.forward
    tails = []
    monkeypatch.setattr(point_ffn, "fused_tail", lambda point, parts, split=False: tails.append(split) or "point_ffn's tail")
    installs = [lambda: point_front.install(P), lambda: point_ffn.install(P, max_channels=512)]
    for step in (installs if front_first else installs[::-1]):
        step()
    try:
        point_ffn.reset_stats()
        point_front.reset_stats()
        block, point = P.Block(c=256), _point(5, 256)
        assert point_front._parts(P.Block(c=128), _point(5, 128), P) is not None    # the width is what turns 256 away
        assert point_front._parts(block, point, P) is None and point_ffn._parts(block, point, P) is not None
        # upstream's front and middle lines, here pass-throughs for a point that holds no tensor
        block.cpe = block.norm1 = block.attn = _Pass()
        point.feat.__class__ = type("Feat", (_FakeCuda,), {"__add__": lambda a, b: a, "__radd__": lambda a, b: a})
        assert block(point) == "point_ffn's tail" and tails == [True]
        assert point_front.stats()["fused_calls"] == 0 and point_ffn.stats()["original_calls"] == 0
    finally:
        order = [point_ffn.uninstall, point_front.uninstall]
        for step in (order if ffn_leaves_first else order[::-1]):
            step(P)
    assert P.Block.forward is own and not [n for n in vars(P) if n.startswith("_gaussiancity_amd")]
