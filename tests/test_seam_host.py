"""The stage-seam operator of libgcm_hip.so and its two Python layers without a GPU (not gpu): the six gcm_seam_* names are in
the header, the binding table and the library's dynamic symbols, and the ABI is still 1; the binding covers every
gcm_seam_* declaration with its argument count; the workspace queries agree with the transcribed plan of
tests/seam_plans.py; every argument error comes back as GCM_ERR_INVALID_ARGUMENT with its message before a device is
touched and an empty problem returns 0; seam.linear_bn_gelu refuses what the library does not run; point_seam on stand-in
containers: which runs are one call and which go the module's own way, the rebound method on the CPU is torch.equal to the
original (features, the sparse tensor's features, the buffers), and install / uninstall restore the functions, in both
orders with point_pool."""
import ctypes as C
import copy
import os
import re
import subprocess
import types

import pytest
import torch
import torch.nn.functional as F

import seam_plans as P
import seam_ref as R
from gaussiancity_amd import _native_m as M
from gaussiancity_amd import point_ffn, point_front, point_mid, point_pool, point_seam, seam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1  # GCM_ERR_INVALID_ARGUMENT
NAMES = {"gcm_seam_max_channels", "gcm_seam_forward_eval", "gcm_seam_forward_workspace_bytes", "gcm_seam_forward_train",
         "gcm_seam_backward_workspace_bytes", "gcm_seam_backward"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gcm.h")).read(), flags=re.S)


def test_the_six_names_are_in_the_header_the_binding_and_the_library_and_the_abi_is_1():
    lib = M.lib()
    assert NAMES <= set(re.findall(r"\b(gcm_[a-z_]+)\s*\(", _header()))
    assert NAMES <= set(M.EXPORTED_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", M.LIB_PATH]).decode()
    assert NAMES <= set(re.findall(r" T (gcm_[a-z_]+)", out))
    assert lib.gcm_abi_version() == 1 and M.ABI_VERSION == 1
    assert "#define GCM_ABI_VERSION 1" in _header()


def test_the_binding_covers_every_seam_declaration_of_the_header_with_its_argument_count():
    declared = dict(re.findall(r"\b(gcm_seam_[a-z_]+)\s*\(([^)]*)\)\s*;", _header()))
    assert set(declared) == NAMES
    for name, args in declared.items():
        count = 0 if args.strip() == "void" else args.count(",") + 1
        assert name in M._SIGNATURES and len(M._SIGNATURES[name][1]) == count, name
        assert getattr(M.lib(), name).argtypes is not None


def test_the_cap_is_512_and_the_python_layer_reports_it():
    assert M.lib().gcm_seam_max_channels() == P.MAX_CHANNELS == seam.max_channels()


def test_the_transcribed_plan_carves_what_the_library_asks_for():
    lib = M.lib()
    for N in (0, 1, 2, 63, 64, 65, 333, 4095, 64 * 64, 64 * 64 + 1, 64 * 64 + 65, 262144, 64 * 64 * 64 + 1):
        for I, O in ((4, 4), (32, 64), (48, 36), (128, 132), (132, 128), (512, 256), (256, 512), (512, 512)):
            p = P.seam_plan(N, I, O)
            assert lib.gcm_seam_forward_workspace_bytes(N, O) == p["forward"], (N, O, p)
            assert lib.gcm_seam_backward_workspace_bytes(N, I, O) == p["total"], (N, I, O, p)
            assert p["forward"] % 256 == 0 and p["forward"] > 0 and p["total"] % 256 == 0
            assert p["G"] <= P.MAX_GROUPS and p["G"] * p["gper"] >= p["tiles"] and p["sw"] <= P.MAX_SLICES
            assert (p["G"] > 1) == (N > 64 * 64)                          # the grouped fold starts beyond 64 tiles
            rows = sum(max(min((s + 1) * p["per"], N) - s * p["per"], 0) for s in range(p["sw"]))
            assert rows == N and p["per"] % P.KC == 0, (N, I, O, p)
    for bad, text in ((0, b"O must be"), (6, b"O must be"), (516, b"above gcm_seam_max_channels")):
        assert lib.gcm_seam_forward_workspace_bytes(10, bad) == 0 and text in lib.gcm_last_error()
        assert lib.gcm_seam_backward_workspace_bytes(10, 8, bad) == 0 and text in lib.gcm_last_error()
    assert lib.gcm_seam_backward_workspace_bytes(10, 6, 8) == 0 and b"I must be" in lib.gcm_last_error()
    assert lib.gcm_seam_backward_workspace_bytes(-1, 8, 8) == 0 and lib.gcm_last_error()


def test_the_workspace_queries_equal_the_transcription_for_every_plan_case():
    lib = M.lib()
    for N, I, O in P.PLAN_CASES:
        p = P.seam_plan(N, I, O)
        assert lib.gcm_seam_forward_workspace_bytes(N, O) == p["forward"], (N, O, p)
        assert lib.gcm_seam_backward_workspace_bytes(N, I, O) == p["total"], (N, I, O, p)
        rows = sum(max(min((s + 1) * p["per"], N) - s * p["per"], 0) for s in range(p["sw"]))
        assert rows == N and p["per"] % P.KC == 0, (N, I, O, p)         # the slices cover every row once
        tiles = sum(max(min((q + 1) * p["gper"], p["tiles"]) - q * p["gper"], 0) for q in range(p["G"]))
        assert tiles == p["tiles"] and (p["G"] - 1) * p["gper"] < p["tiles"], (N, I, O, p)   # and the groups every tile
    assert set(P.NO_PRODUCT_CASES) <= set(P.PLAN_CASES) and set(P.STATISTICS_CASES) <= set(P.NO_PRODUCT_CASES)


@pytest.mark.parametrize("shape", sorted(P.PLAN_CASES))
def test_every_plan_case_reaches_the_branch_it_names(shape):
    stated, derived = P.PLAN_CASES[shape], P.facts(shape)
    assert stated and set(stated) <= set(derived)
    wrong = {k: (v, derived[k]) for k, v in stated.items() if derived[k] != v}
    assert not wrong, (shape, wrong)


@pytest.mark.parametrize("name", [n for n, _ in P.BRANCH_FACTS])
def test_every_branch_fact_is_held_by_a_plan_case(name):
    holds = dict(P.BRANCH_FACTS)[name]
    assert [shape for shape in P.PLAN_CASES if holds(P.facts(shape))], name


def test_the_drift_and_momentum_knobs_default_to_the_inputs_and_the_formulation_they_had():
    for product in (True, False):
        a, b = R.make_inputs(70, 8, 12, 5, product), R.make_inputs(70, 8, 12, 5, product, drift=50.0)
        col = 0 if product else 2
        ramp = torch.linspace(0, 50.0, 70)
        assert torch.equal(b["x"][:, col], a["x"][:, col] + ramp)
        b["x"][:, col] = a["x"][:, col]
        assert all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in a)
    inp = R.make_inputs(70, 8, 12, 5)
    plain, full = (R.run(R.torch_ops, inp, "cpu", torch.float64, True, True, **kw)[0] for kw in ({}, {"momentum": 1.0}))
    z = F.linear(inp["x"].double(), inp["w"].double(), inp["b"].double())
    assert torch.allclose(full["running_mean"], z.mean(0), rtol=1e-12, atol=1e-12)
    assert torch.allclose(full["running_var"], z.var(0, unbiased=True), rtol=1e-12, atol=1e-12)
    want = 0.99 * inp["running_mean"].double() + 0.01 * z.mean(0)
    assert torch.allclose(plain["running_mean"], want, rtol=1e-12, atol=1e-12) and torch.equal(plain["y"], full["y"])


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


def _eval(lib, p, xs=8, ys=8, N=4, I=8, O=8, eps=1e-3, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    return lib.gcm_seam_forward_eval(g("x"), xs, g("w"), g("b"), g("running_mean"), g("running_var"), eps, g("bn_w"),
                                     g("bn_b"), 1, N, I, O, g("y"), ys, ptr.get("z"), ptr.get("rstd"), None)


def _train(lib, p, xs=8, ys=8, N=4, I=8, O=8, eps=1e-3, momentum=0.01, work="p", bytes_=None, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    need = lib.gcm_seam_forward_workspace_bytes(N, O) if bytes_ is None else bytes_
    return lib.gcm_seam_forward_train(g("x"), xs, g("w"), g("b"), eps, momentum, g("bn_w"), g("bn_b"), 1, N, I, O, g("z"),
                                      g("y"), ys, g("mean"), g("rstd"), g("running_mean"), g("running_var"), g("tracked"),
                                      p if work == "p" else work, need, None)


def _backward(lib, p, xs=8, zs=8, dys=8, dxs=8, N=4, I=8, O=8, batch=1, work="p", bytes_=None, **ptr):
    g = lambda k: ptr.get(k, p)  # noqa: E731
    need = lib.gcm_seam_backward_workspace_bytes(N, I, O) if bytes_ is None else bytes_
    return lib.gcm_seam_backward(g("x"), xs, g("z"), zs, g("mean"), g("rstd"), g("dy"), dys, g("w"), g("bn_w"), g("bn_b"), 1,
                                 batch, N, I, O, g("dx"), dxs, g("dw"), g("db"), g("dbn_w"), g("dbn_b"),
                                 p if work == "p" else work, need, None)


def test_every_refusal_is_made_before_a_device_call_each_with_its_message(mem):
    lib, _, p = mem
    wide = lib.gcm_seam_max_channels() + 4
    big = 1 << 30
    for call in (_eval, _train, _backward):
        kw = {"bytes_": big} if call is not _eval else {}
        _refused(lib, call(lib, p, O=0, **kw), b"O must be")                                       # width 0
        _refused(lib, call(lib, p, I=0, **kw), b"I must be")
        _refused(lib, call(lib, p, O=6, **kw), b"O must be")                                       # no multiple of 4
        _refused(lib, call(lib, p, I=6, **kw), b"I must be")
        _refused(lib, call(lib, p, O=wide, **kw), b"above gcm_seam_max_channels")                  # beyond the cap
        _refused(lib, call(lib, p, I=wide, xs=wide, **kw), b"above gcm_seam_max_channels")
        _refused(lib, call(lib, p, w=None, b=None, I=8, O=12, ys=12, **kw), b"w == NULL needs I == O")
        _refused(lib, call(lib, p, N=-1, **kw), b"N out of range")
        _refused(lib, call(lib, p, N=1 << 31, **kw), b"N out of range")
        for bad in (6, 0, -8, 4):
            _refused(lib, call(lib, p, xs=bad, **kw), b"strides")
        _refused(lib, call(lib, p, x=p + 4), b"16-byte")                                           # a misaligned pointer
        _refused(lib, call(lib, p, bn_w=p + 8), b"16-byte")
    _refused(lib, _train(lib, p, N=1), b"batch statistics need N >= 2")                            # torch raises there
    _refused(lib, _backward(lib, p, N=1), b"batch statistics need N >= 2")
    none = dict(dw=None, db=None, dbn_w=None, dbn_b=None)
    assert _backward(lib, p, N=0, **none) == 0 and _train(lib, p, N=0) == 0 and _eval(lib, p, N=0) == 0    # N == 0 queues nothing
    _refused(lib, _train(lib, p, tracked=p + 4), b"8-byte")
    _refused(lib, _train(lib, p, tracked=None), b"all or none")
    _refused(lib, _train(lib, p, w=None), b"need w")
    _refused(lib, _eval(lib, p, w=None), b"need w")
    _refused(lib, _backward(lib, p, w=None), b"need w")
    for bad in (float("nan"), -1.0):
        _refused(lib, _eval(lib, p, eps=bad), b"eps must be")
        _refused(lib, _train(lib, p, eps=bad), b"eps must be")
    _refused(lib, _train(lib, p, momentum=1.5), b"momentum")
    for name in ("x", "bn_w", "bn_b", "y", "running_mean", "running_var"):
        _refused(lib, _eval(lib, p, **{name: None}), b"null")
    for name in ("x", "bn_w", "bn_b", "y", "mean", "rstd", "z"):
        _refused(lib, _train(lib, p, **{name: None}), b"null")
    for name in ("x", "z", "mean", "rstd", "dy", "bn_w", "bn_b"):
        _refused(lib, _backward(lib, p, **{name: None}), b"null")
    for call, query in ((_train, lib.gcm_seam_forward_workspace_bytes(4, 8)), (_backward, lib.gcm_seam_backward_workspace_bytes(4, 8, 8))):
        assert query > 0
        _refused(lib, call(lib, p, bytes_=query - 1), b"workspace smaller")                        # a short workspace
        _refused(lib, call(lib, p, work=None), b"workspace smaller")
        _refused(lib, call(lib, p, work=p + 16), b"256-byte")


# ---- the Python operator --------------------------------------------------------------------------------------------------
def _args(inp):
    return (inp["x"], inp["w"], inp["b"], inp["g"], inp["h"], inp["running_mean"], inp["running_var"], inp["tracked"])


def test_the_operator_refuses_what_the_library_does_not_run():
    inp = R.make_inputs(5, 8, 12, 1)
    kw = dict(training=True, momentum=0.01, eps=1e-3)
    with pytest.raises(TypeError, match="CUDA"):
        seam.linear_bn_gelu(*_args(inp), **kw)
    with pytest.raises(ValueError, match=r"x must be \[N, I\]"):
        seam.linear_bn_gelu(inp["x"][0], *_args(inp)[1:], **kw)
    with pytest.raises(ValueError, match="multiple of 4"):
        seam.linear_bn_gelu(inp["x"][:, :6], inp["w"][:, :6], *_args(inp)[2:], **kw)
    with pytest.raises(ValueError, match="multiple of 4"):
        seam.linear_bn_gelu(torch.zeros(5, 0), torch.zeros(12, 0), *_args(inp)[2:], **kw)
    wide = seam.max_channels() + 4
    with pytest.raises(ValueError, match="hold I up to"):
        seam.linear_bn_gelu(torch.zeros(5, wide), torch.zeros(12, wide), *_args(inp)[2:], **kw)
    with pytest.raises(ValueError, match="hold O up to"):
        seam.linear_bn_gelu(inp["x"], torch.zeros(wide, 8), *_args(inp)[2:], **kw)
    with pytest.raises(TypeError, match="float32"):
        seam.linear_bn_gelu(inp["x"].half(), *_args(inp)[1:], **kw)
    with pytest.raises(TypeError, match="float32"):
        seam.linear_bn_gelu(inp["x"], inp["w"].double(), *_args(inp)[2:], **kw)
    with pytest.raises(ValueError, match="bn_weight must be"):
        seam.linear_bn_gelu(inp["x"], inp["w"], inp["b"], inp["g"][:8], *_args(inp)[4:], **kw)
    with pytest.raises(ValueError, match="bias needs weight"):
        seam.linear_bn_gelu(inp["x"], None, inp["b"], *_args(inp)[3:], **kw)
    with pytest.raises(ValueError, match="bn_weight must be"):          # no product: O is I
        seam.linear_bn_gelu(inp["x"], None, None, *_args(inp)[3:], **kw)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        seam.linear_bn_gelu(inp["x"][:1], *_args(inp)[1:], **kw)
    with pytest.raises(ValueError, match="momentum"):
        seam.linear_bn_gelu(*_args(inp), training=True, momentum=None, eps=1e-3)
    with pytest.raises(ValueError, match="eps"):
        seam.linear_bn_gelu(*_args(inp), training=True, momentum=0.1, eps=-1.0)
    with pytest.raises(TypeError, match="int64"):
        seam.linear_bn_gelu(*_args(inp)[:7], inp["tracked"].int(), **kw)
    with pytest.raises(ValueError, match="all or none"):
        seam.linear_bn_gelu(*_args(inp)[:7], None, **kw)
    with pytest.raises(ValueError, match="eval mode reads"):
        seam.linear_bn_gelu(*_args(inp)[:5], None, None, None, training=False, momentum=0.01, eps=1e-3)


# ---- point_seam on stand-in containers ------------------------------------------------------------------------------------
class _Sparse:
    """spconv.SparseConvTensor's features and replace_feature."""
    def __init__(self, features):
        self.features = features

    def replace_feature(self, features):
        return _Sparse(features)


def _stand_in():
    """What install() needs of models/pt_v3.py, written for this test: Point (a dict with attributes), PointModule, a
    PointSequential whose forward is the walk the module documents, a spconv namespace that knows its convolution, and the
    two pooling classes point_pool rebinds."""
    class Point(dict):
        __getattr__ = dict.__getitem__
        __setattr__ = dict.__setitem__

    class PointModule(torch.nn.Module):
        pass

    class Conv(torch.nn.Module):
        def forward(self, s):
            return s.replace_feature(s.features * 2.0)

    spconv = types.SimpleNamespace(modules=types.SimpleNamespace(is_spconv_module=lambda m: isinstance(m, Conv)))

    class PointSequential(PointModule):
        def __init__(self, *mods):
            super().__init__()
            for i, mod in enumerate(mods):
                self.add_module(str(i), mod)

        def forward(self, x):
            for module in self._modules.values():
                if isinstance(module, PointModule):
                    x = module(x)
                elif spconv.modules.is_spconv_module(module):
                    x.sparse_conv_feat = module(x.sparse_conv_feat)
                    x.feat = x.sparse_conv_feat.features
                elif isinstance(module, torch.nn.BatchNorm1d) and isinstance(x, Point):
                    if x.feat.size(0) != 1:
                        x.feat = module(x.feat)
                elif isinstance(x, Point):
                    x.feat = module(x.feat)
                    if "sparse_conv_feat" in x.keys():
                        x.sparse_conv_feat = x.sparse_conv_feat.replace_feature(x.feat)
                else:
                    x = module(x)
            return x

    class Block(PointModule):
        def forward(self, point):
            return "block"

    class SerializedPooling(PointModule):
        def forward(self, point):
            return "pooling"

    class SerializedUnpooling(PointModule):
        def forward(self, point):
            return "unpooling"

    return types.SimpleNamespace(Point=Point, PointModule=PointModule, PointSequential=PointSequential, Conv=Conv, spconv=spconv,
                                 Block=Block, SerializedPooling=SerializedPooling, SerializedUnpooling=SerializedUnpooling)


class _FakeCuda:
    """A feature tensor's stand-in that says it is on the GPU: the checks that come after the device are reached here."""
    is_cuda = True

    def __init__(self, n, c, dtype=torch.float32):
        self.shape, self.dtype = (n, c), dtype

    def dim(self):
        return 2


def _bn(c, **kw):
    return torch.nn.BatchNorm1d(c, eps=1e-3, momentum=kw.pop("momentum", 0.01), **kw)


def test_which_runs_are_one_call_and_which_go_the_modules_own_way(monkeypatch):
    S = _stand_in()
    lin, gelu = torch.nn.Linear, torch.nn.GELU
    point = lambda n=5, c=16, dtype=torch.float32, **k: S.Point(feat=_FakeCuda(n, c, dtype), **k)  # noqa: E731
    taken = lambda mods, pt, i=0: point_seam._run_at(list(mods), i, pt)  # noqa: E731
    accepted = {
        "Linear, norm, GELU": ((lin(16, 32), _bn(32), gelu()), point(), 3),
        "norm, GELU (the stem's tail, the pooling pair)": ((_bn(16), gelu()), point(), 2),
        "a lone norm": ((_bn(16),), point(), 1),
        "Linear, norm without the key": ((lin(16, 32), _bn(32)), point(), 2),
        "Linear without bias": ((lin(16, 32, bias=False), _bn(32), gelu()), point(), 3),
        "the sparse key with a GELU at the end": ((lin(16, 32), _bn(32), gelu()), point(sparse_conv_feat=None), 3),
        "a lone norm with the key": ((_bn(16),), point(sparse_conv_feat=None), 1),
        "the cap itself": ((lin(16, 512), _bn(512), gelu()), point(), 3),
        "a tanh GELU stays outside the run": ((_bn(16), gelu(approximate="tanh")), point(), 1),
        "an eval-mode norm": ((lin(16, 32), _bn(32).eval(), gelu()), point(), 3),
    }
    for why, (mods, pt, length) in accepted.items():
        run = taken(mods, pt)
        assert run is not None and run[3] == length, why
    declined = {
        "another module type": ((torch.nn.LayerNorm(16), gelu()), point()),
        "a Linear that no norm follows": ((lin(16, 16), gelu()), point()),
        "one row: upstream skips the norm": ((lin(16, 32), _bn(32), gelu()), point(n=1)),
        "no row": ((_bn(16), gelu()), point(n=0)),
        "CPU tensors": ((lin(16, 32), _bn(32), gelu()), S.Point(feat=torch.zeros(5, 16))),
        "float16 features": ((_bn(16), gelu()), point(dtype=torch.float16)),
        "float64 features": ((_bn(16), gelu()), point(dtype=torch.float64)),
        "a width beyond the cap": ((_bn(516), gelu()), point(c=516)),
        "an input width beyond the cap": ((lin(516, 16), _bn(16)), point(c=516)),
        "a width that is no multiple of 4": ((_bn(18), gelu()), point(c=18)),
        "an input width that is no multiple of 4": ((lin(18, 16), _bn(16)), point(c=18)),
        "affine=False": ((_bn(16, affine=False), gelu()), point()),
        "track_running_stats=False": ((_bn(16, track_running_stats=False), gelu()), point()),
        "momentum=None": ((_bn(16, momentum=None), gelu()), point()),
        "Linear, norm and no GELU while the sparse key is present": ((lin(16, 32), _bn(32)), point(sparse_conv_feat=None)),
        "a norm of another width than the Linear": ((lin(16, 32), _bn(16), gelu()), point()),
        "a Linear subclass": ((type("L", (lin,), {})(16, 32), _bn(32)), point()),
        "a BatchNorm1d subclass": ((type("B", (torch.nn.BatchNorm1d,), {})(16), gelu()), point()),
    }
    for why, (mods, pt) in declined.items():
        assert taken(mods, pt) is None, why
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    assert taken((_bn(16), gelu()), point()) is None, "active autocast"


def test_a_non_point_input_and_a_container_without_a_norm_go_to_the_modules_own_method_whole():
    S = _stand_in()
    point_seam.install(S)
    try:
        point_seam.reset_stats()
        x = torch.randn(5, 16)
        seq = S.PointSequential(torch.nn.Linear(16, 16), _bn(16), torch.nn.GELU())
        ref = copy.deepcopy(seq)
        assert torch.equal(seq(x), getattr(S, point_seam._ORIGINAL)(ref, x))
        assert point_seam.stats()["original_calls"] == 1 and point_seam.stats()["fused_runs"] == 0
        S.PointSequential(torch.nn.Linear(16, 16), torch.nn.GELU())(S.Point(feat=x))
        assert point_seam.stats()["original_calls"] == 2 and point_seam.stats()["original_modules"] == 0
    finally:
        point_seam.uninstall(S)


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("rows", (5, 1))
def test_on_the_cpu_the_rebound_method_is_torch_equal_to_the_original(training, rows):
    S = _stand_in()
    torch.manual_seed(3)
    inner = S.PointSequential(_bn(32), torch.nn.GELU())
    seq = S.PointSequential(S.Conv(), torch.nn.Linear(16, 32), _bn(32), torch.nn.GELU(), inner, torch.nn.Linear(32, 32), _bn(32))
    with torch.no_grad():
        for mod in seq.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.normal_()
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.normal_()
    seq.train(training)
    ref = copy.deepcopy(seq)
    x = torch.randn(rows, 16)

    def go(s):
        pt = S.Point(feat=x.clone().requires_grad_(True), sparse_conv_feat=_Sparse(x.clone()))
        out = s(pt)
        out.feat.sum().backward()
        return out

    want = go(ref)
    point_seam.install(S)
    try:
        point_seam.reset_stats()
        got = go(seq)
        st = point_seam.stats()
    finally:
        point_seam.uninstall(S)
    assert torch.equal(got.feat, want.feat) and torch.equal(got.sparse_conv_feat.features, want.sparse_conv_feat.features)
    if rows != 1:      # the last norm's branch leaves the key behind; with one row upstream skips the norm
        assert not torch.equal(got.feat, got.sparse_conv_feat.features)
    for (name, a), (_, b) in zip(seq.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), name
    for a, b in zip(seq.parameters(), ref.parameters()):
        assert (a.grad is None and b.grad is None) or torch.equal(a.grad, b.grad)
    assert st["fused_runs"] == 0 and st["original_modules"] == 7 + 2 and st["original_calls"] == 0


def test_install_and_uninstall_are_idempotent_and_restore_the_method():
    S = _stand_in()
    own = S.PointSequential.forward
    point_seam.uninstall(S)  # nothing installed: nothing happens
    assert S.PointSequential.forward is own
    point_seam.install(S)
    bound = S.PointSequential.forward
    assert bound is not own and getattr(S, point_seam._MARK) is True
    point_seam.install(S)
    assert S.PointSequential.forward is bound and getattr(S, point_seam._ORIGINAL) is own
    point_seam.uninstall(S)
    assert S.PointSequential.forward is own and not [n for n in vars(S) if n.startswith("_gaussiancity_amd")]
    point_seam.uninstall(S)
    assert S.PointSequential.forward is own


@pytest.mark.parametrize("install_order", ("pool, seam", "seam, pool"))
@pytest.mark.parametrize("uninstall_order", ("pool, seam", "seam, pool"))
def test_point_pool_and_point_seam_compose_in_either_order(install_order, uninstall_order):
    S = _stand_in()
    own = (S.PointSequential.forward, S.SerializedPooling.forward, S.SerializedUnpooling.forward)
    mods = {"pool": point_pool, "seam": point_seam}
    for name in install_order.split(", "):
        mods[name].install(S)
    assert S.PointSequential.forward is not own[0] and S.SerializedPooling.forward is not own[1]
    for name in install_order.split(", "):      # idempotent while both are bound
        before = (S.PointSequential.forward, S.SerializedPooling.forward)
        mods[name].install(S)
        assert (S.PointSequential.forward, S.SerializedPooling.forward) == before
    first, second = uninstall_order.split(", ")
    mods[first].uninstall(S)
    mods[second].uninstall(S)
    assert (S.PointSequential.forward, S.SerializedPooling.forward, S.SerializedUnpooling.forward) == own
    assert not [n for n in vars(S) if n.startswith("_gaussiancity_amd")]


@pytest.mark.parametrize("order", ("pool, front, mid, ffn, seam", "seam, ffn, mid, front, pool", "mid, seam, pool, ffn, front"))
def test_all_five_installs_compose_and_every_method_comes_back(order):
    S = _stand_in()
    own = (S.PointSequential.forward, S.Block.forward, S.SerializedPooling.forward, S.SerializedUnpooling.forward)
    mods = {"pool": point_pool, "front": point_front, "mid": point_mid, "ffn": point_ffn, "seam": point_seam}
    names = order.split(", ")
    for name in names:
        mods[name].install(S)
    assert S.PointSequential.forward is not own[0] and S.Block.forward is not own[1] and S.SerializedPooling.forward is not own[2]
    assert getattr(S, point_seam._MARK) is True
    for name in names:
        mods[name].uninstall(S)
    for name in reversed(names):      # idempotent: a second round finds nothing to remove
        mods[name].uninstall(S)
    assert (S.PointSequential.forward, S.Block.forward, S.SerializedPooling.forward, S.SerializedUnpooling.forward) == own
    assert not [n for n in vars(S) if n.startswith("_gaussiancity_amd")]


def test_the_pooling_tail_takes_exactly_the_pair():
    S = _stand_in()
    pt = lambda: S.Point(feat=_FakeCuda(5, 16))  # noqa: E731
    seq = S.PointSequential
    assert not point_seam.pooling_tail(seq(_bn(16), torch.nn.GELU()), seq(torch.nn.GELU()), pt())     # two modules in norm
    assert not point_seam.pooling_tail(seq(_bn(16)), seq(torch.nn.ReLU()), pt())                      # another activation
    assert not point_seam.pooling_tail(seq(torch.nn.LayerNorm(16)), seq(torch.nn.GELU()), pt())       # another norm
    assert not point_seam.pooling_tail(seq(_bn(16)), seq(torch.nn.GELU()), S.Point(feat=torch.zeros(5, 16)))   # CPU
    assert not point_seam.pooling_tail(seq(_bn(16, affine=False)), seq(torch.nn.GELU()), pt())
