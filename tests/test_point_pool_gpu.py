"""SerializedPooling / SerializedUnpooling on the device (include/gcs.h, gaussiancity_amd/point_pool.py, DESIGN.md section
15.6).

The plan is integer work: bit-exact against tests/pool_ref.py and against the keys the reference recorded.  The gathered
reduce has segment_csr's numerics and is compared with `segment_csr(src[indices], indptr)` by torch.equal; independently
of that kernel, sum and mean are held to the project's bars of a float64 evaluation: 1e-5 * sum|terms| in float32,
2^-11 * sum|terms| + 2^-24 in float16.  The rebound modules are compared with the reference's own float64 run, per tensor
within 4 x the error of the reference's own float32 run (tests/golden/ptv3_pool.npz), the scheme and the margin of
tests/test_attr_head_gpu.py: the products in front of the reduce are rocBLAS's on both sides.

Measured on the MI355X, the rebound pair's worst tensor per case as a fraction of the tensor's maximum (the reference's own
float32 run in brackets): (a) 4.3e-7 (3.8e-7), (b) 5.1e-7 (6.5e-7), (c) 5.8e-7 (4.9e-7); the worst ratio of a tensor's error to
the reference's float32 error is 2.6, under the bar of 4.
"""
import functools
import os
import types

import numpy as np
import pytest
import torch

import pool_ref as R
from gaussiancity_amd import _native_s as S
from gaussiancity_amd import point_pool as PP
from gaussiancity_amd.sparse import segment_csr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCES = ("sum", "mean", "min", "max")
DTYPES = {"float32": torch.float32, "float16": torch.float16}
WIDTHS = (1, 3, 4, 5, 32, 36, 64, 68, 512)
SEGMENTS = (1, 7, 64, 65)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ptv3_pool.npz"))


# ---------------------------------------------------------------------------------------------- the plan
def _codes(rng, pattern, n, k, shift):
    if pattern == "mixed":      # three batches above bit 42, a few rows per cluster, some codes negative
        row0 = (rng.integers(0, 3, n) << 42 | rng.integers(0, 4096, n)) - 2000
    elif pattern == "one":      # all rows in one cluster
        row0 = np.full(n, 7 << 42 | 5)
    elif pattern == "distinct":  # every key its own cluster, rows in no order
        row0 = rng.permutation(n) << shift | rng.integers(0, 1 << shift, n)
    else:                       # "batch": keys that differ only above bit 40
        row0 = rng.integers(0, 5, n) << 41 | 3
    rows = [row0] + [rng.integers(0, 8, n) << shift | rng.integers(0, 1 << shift, n) for _ in range(k - 1)]
    return np.stack(rows).astype(np.int64)   # rows 1...: eight values after the shift, so down_code is full of ties


def _check_plan(dev, code, depth):
    plan = PP.pool_plan(torch.from_numpy(code).to(dev), depth)
    want = R.plan(code, 3 * depth)
    assert (plan.n, plan.s) == (want.n, want.s)
    for name in ("cluster", "indices", "idx_ptr", "head", "code", "order", "inverse"):
        got = getattr(plan, name)
        assert got.dtype == torch.int64 and got.device.type == "cuda", name
        assert np.array_equal(got.cpu().numpy(), getattr(want, name)), name
    return plan


@pytest.mark.parametrize("shift", [0, 3, 9])
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097])
def test_plan_is_bit_exact(cuda_device, n, k, shift):
    rng = np.random.default_rng(1000 * n + 10 * k + shift)
    for pattern in ("mixed", "one", "distinct", "batch"):
        _check_plan(cuda_device, _codes(rng, pattern, n, k, shift), shift // 3)


def test_plan_ties_in_a_cord_row_go_to_the_lower_position(cuda_device):
    """A `cord` row of the pooled set with equal codes, input rows not in code order, and the deepest shift."""
    code = np.array([[40, 8, 41, 8, 16, 9, 40, 0, 17]], np.int64)   # >> 3: 5 1 5 1 2 1 5 0 2
    plan = _check_plan(cuda_device, code, 1)
    assert plan.head.tolist() == [7, 1, 4, 0] and plan.indices.tolist() == [7, 1, 3, 5, 4, 8, 0, 2, 6]
    two = np.stack([code[0], np.array([3, 8, 3, 3, 9, 3, 3, 8, 3])]).astype(np.int64)   # row 1 at the heads: 1 1 1 0
    plan = _check_plan(cuda_device, two, 1)
    assert plan.code[1].tolist() == [1, 1, 1, 0] and plan.order[1].tolist() == [3, 0, 1, 2]
    _check_plan(cuda_device, (np.arange(50, dtype=np.int64)[None] % 7) << 48, 16)


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_plan_equals_the_reference_run(cuda_device, golden, case):
    g = lambda k: golden["%s.int.%s" % (case, k)]  # noqa: E731
    d = {"a": 1, "b": 1, "c": 0}[case]
    plan = _check_plan(cuda_device, g("in.serialized_code"), d)
    for name, key in (("cluster", "pooling_inverse"), ("code", "serialized_code"), ("order", "serialized_order"),
                      ("inverse", "serialized_inverse")):
        assert np.array_equal(getattr(plan, name).cpu().numpy(), g(key)), key
    head = plan.head.cpu().numpy()
    assert np.array_equal(golden[case + ".grid"][head] >> d, g("grid_coord")) and np.array_equal(golden["batch"][head], g("batch"))


# ---------------------------------------------------------------------------------------------- the gathered reduce
def _sizes(s):
    """Segment sizes mixing 1, 2, 8, 65, 300 and an empty segment."""
    if s == 1:
        return [300]
    base = [1, 2, 8, 0, 65, 300, 3]
    return base + [(1, 2, 8, 0, 3)[i % 5] for i in range(s - len(base))]


def _hand_plan(dev, s, seed):
    sizes = np.array(_sizes(s), np.int64)
    m = int(sizes.sum())
    idx_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    indices = np.random.default_rng(seed).permutation(m).astype(np.int64)
    cluster = np.empty(m, np.int64)
    cluster[indices] = R.segments(idx_ptr, m)
    head = indices[np.minimum(idx_ptr[:-1], m - 1)]
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    z = torch.zeros((1, s), dtype=torch.int64, device=dev)
    return PP.PoolPlan(t(cluster), t(indices), t(idx_ptr), t(head), z, z, z, m, s)


def _csr(src, indptr, reduce):
    """(out, arg) of the library's segment_csr kernel; arg is None for sum and mean."""
    out = segment_csr(src, indptr, reduce=reduce)
    if reduce in ("sum", "mean"):
        return out, None
    m, f, s = src.shape[0], src.shape[1], indptr.numel() - 1
    arg = torch.empty((s, f), dtype=torch.int64, device=src.device)
    out2 = torch.empty_like(out)
    S.check(S.lib().gcs_segment_csr_forward_t(S.DTYPES[str(src.dtype).split(".")[1]], src.data_ptr(), m, f, indptr.data_ptr(), s,
                                              S.REDUCE[reduce], out2.data_ptr(), arg.data_ptr(), None), "gcs_segment_csr_forward_t")
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    return out, arg


def _source(dev, m, f, dtype, seed, ties):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (m, f), generator=g).float() if ties else torch.randn(m, f, generator=g)
    return x.to(dtype).to(dev)


def _bars(x, plan, got, reduce, dtype):
    """sum and mean against a float64 evaluation that shares nothing with the kernels."""
    gathered = x.double()[plan.indices]
    seg = torch.repeat_interleave(torch.arange(plan.s, device=x.device), plan.idx_ptr[1:] - plan.idx_ptr[:-1])
    want = torch.zeros((plan.s, x.shape[1]), dtype=torch.float64, device=x.device).index_add_(0, seg, gathered)
    mass = torch.zeros_like(want).index_add_(0, seg, gathered.abs())
    if reduce == "mean":
        cnt = (plan.idx_ptr[1:] - plan.idx_ptr[:-1]).clamp(min=1).double().unsqueeze(1)
        want, mass = want / cnt, mass / cnt
    bar = 1e-5 * mass if dtype == torch.float32 else 2.0 ** -11 * mass + 2.0 ** -24
    excess = ((got.double() - want).abs() - bar).max().item()
    assert excess <= 0, (reduce, dtype, excess)


@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_gather_forward_equals_segment_csr_of_the_gathered_copy(cuda_device, dtype, f):
    dt = DTYPES[dtype]
    for s in SEGMENTS:
        plan = _hand_plan(cuda_device, s, 100 * f + s)
        for ties in (False, True):
            x = _source(cuda_device, plan.n, f, dt, f + s, ties)
            gathered = x[plan.indices]
            for reduce in REDUCES:
                want, want_arg = _csr(gathered, plan.idx_ptr, reduce)
                got, arg = PP.gather_forward(x, plan, reduce)
                assert got.dtype == dt and torch.equal(got, want), (s, reduce, ties)
                if want_arg is None:
                    assert arg is None
                    if not ties:
                        _bars(x, plan, got, reduce, dt)
                else:   # the arg is a SOURCE row: segment_csr's position mapped through indices, -1 kept
                    mapped = torch.where(want_arg >= 0, plan.indices[want_arg.clamp(min=0)], want_arg)
                    assert torch.equal(arg, mapped), (s, reduce, ties)
                    assert (arg[plan.idx_ptr[1:] == plan.idx_ptr[:-1]] == -1).all()
                assert torch.equal(PP.pooled_reduce(x, plan, reduce), want)
        # rows strided in place (a column slice of a wider tensor), and a base address one element off
        wide = _source(cuda_device, plan.n, f + 8, dt, 7, False)
        for start in (4 if dt == torch.float32 else 8, 1):
            view = wide[:, start:start + f]
            for reduce in REDUCES:
                a, arg_a = PP.gather_forward(view, plan, reduce)
                b, arg_b = PP.gather_forward(view.contiguous(), plan, reduce)
                assert torch.equal(a, b) and (arg_a is None or torch.equal(arg_a, arg_b)), (s, reduce, start)


@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_gather_backward_and_expand_add(cuda_device, dtype, f):
    dt = DTYPES[dtype]
    for s in SEGMENTS:
        plan = _hand_plan(cuda_device, s, 200 * f + s)
        g = torch.Generator().manual_seed(s)
        dout = torch.randn(plan.s, f, generator=g).to(dt).to(cuda_device)
        for reduce in REDUCES:
            x = _source(cuda_device, plan.n, f, dt, 3 * f + s, reduce in ("min", "max")).requires_grad_(True)
            ref = x.detach().clone().requires_grad_(True)
            segment_csr(ref[plan.indices], plan.idx_ptr, reduce=reduce).backward(dout)
            PP.pooled_reduce(x, plan, reduce).backward(dout)
            assert x.grad.dtype == dt and torch.equal(x.grad, ref.grad), (s, reduce)
            first = x.grad.clone()
            x.grad = None
            PP.pooled_reduce(x, plan, reduce).backward(dout)
            assert torch.equal(x.grad, first)   # run to run
            if reduce in ("min", "max"):   # with ties present, the first attaining row of a segment has the gradient
                _, arg = PP.gather_forward(x.detach(), plan, reduce)
                col = torch.arange(f, device=cuda_device).expand_as(arg)
                live = arg >= 0
                want = torch.zeros_like(first)
                want[arg[live], col[live]] = dout[live]
                assert torch.equal(first, want)
            # a buffer full of NaN comes back fully overwritten: every element is written, nothing is cleared first
            _, arg = PP.gather_forward(x.detach(), plan, reduce)
            buf = torch.full((plan.n, f), float("nan"), dtype=dt, device=cuda_device)
            out = PP.gather_backward(dout, plan, reduce, arg, out=buf)
            assert out is buf and not torch.isnan(buf).any() and torch.equal(buf, first)
        # expand_add: one fp32 add, rounded once -- in float32 torch's own a + b[cluster] bit for bit
        a = _source(cuda_device, plan.n, f, dt, 5, False).requires_grad_(True)
        b = _source(cuda_device, plan.s, f, dt, 6, False).requires_grad_(True)
        out = PP.unpool_add(a, b, plan)
        want = (a.detach().float() + b.detach().float()[plan.cluster]).to(dt)
        assert torch.equal(out, want)
        if dt == torch.float32:
            assert torch.equal(out, a.detach() + b.detach()[plan.cluster])
        assert torch.equal(PP.unpool_add(None, b.detach(), plan), b.detach()[plan.cluster])
        up = torch.randn(plan.n, f, generator=g).to(dt).to(cuda_device)
        out.backward(up)
        d_b = segment_csr(up[plan.indices], plan.idx_ptr, reduce="sum")
        assert torch.equal(a.grad, up) and torch.equal(b.grad, d_b)
        _bars(up, plan, b.grad, "sum", dt)
        first = b.grad.clone()
        a.grad = b.grad = None
        PP.unpool_add(a, b, plan).backward(up)
        assert torch.equal(b.grad, first)


def test_a_segment_of_thousands_of_rows(cuda_device):
    """One cluster of 5000 rows next to single rows: legal, and still segment_csr's chain."""
    sizes = np.array([1, 5000, 1, 2], np.int64)
    m = int(sizes.sum())
    idx_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    indices = np.random.default_rng(3).permutation(m).astype(np.int64)
    cluster = np.empty(m, np.int64)
    cluster[indices] = R.segments(idx_ptr, m)
    t = lambda a: torch.from_numpy(a).to(cuda_device)  # noqa: E731
    z = torch.zeros((1, 4), dtype=torch.int64, device=cuda_device)
    plan = PP.PoolPlan(t(cluster), t(indices), t(idx_ptr), t(indices[idx_ptr[:-1]]), z, z, z, m, 4)
    x = _source(cuda_device, m, 36, torch.float32, 9, False)
    for reduce in REDUCES:
        assert torch.equal(PP.gather_forward(x, plan, reduce)[0], segment_csr(x[plan.indices], plan.idx_ptr, reduce=reduce))


def test_reduce_and_unpool_never_wait(cuda_device):
    """pooled_reduce and unpool_add, forward and backward, under torch.cuda.set_sync_debug_mode("error")."""
    plan = _hand_plan(cuda_device, 65, 1)
    x = _source(cuda_device, plan.n, 36, torch.float32, 1, False).requires_grad_(True)
    a = _source(cuda_device, plan.n, 36, torch.float32, 2, False).requires_grad_(True)
    b = _source(cuda_device, plan.s, 36, torch.float32, 3, False).requires_grad_(True)
    dout, up = torch.ones(plan.s, 36, device=cuda_device), torch.ones(plan.n, 36, device=cuda_device)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for reduce in REDUCES:
            PP.pooled_reduce(x, plan, reduce).backward(dout)
        PP.unpool_add(a, b, plan).backward(up)
        flagged = False
        try:
            x.sum().item()
        except RuntimeError:
            flagged = True
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert flagged, "this torch build does not flag .item() under set_sync_debug_mode('error'): the test shows nothing"
    assert x.grad is not None and b.grad is not None


# ---------------------------------------------------------------------------------------------- the rebound modules
class _Dict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _stand_in():
    """What install() needs of models/pt_v3.py, written for this test from the modules' behaviour.  The pooling's own
    forward raises; the unpooling's own forward is upstream's gather and add, which the test reaches on purpose."""

    class Point(_Dict):
        def sparsify(self, pad=96):
            self["sparsified"] = True

    class PointSequential(torch.nn.Module):
        """Upstream's constructor is (name="", *modules): a first module handed over positionally lands in `name`, which
        is where the recorded state dicts have it ("norm.name.weight", "proj.name.weight", then "proj.1", "proj.2")."""

        def __init__(self, name="", *modules):
            super().__init__()
            self.name = name
            for m in modules:
                self.add(m)

        def add(self, module):
            self.add_module(str(len(self._modules)), module)

        def forward(self, point):
            for m in self._modules.values():
                if not (isinstance(m, torch.nn.BatchNorm1d) and point.feat.size(0) == 1):
                    point.feat = m(point.feat)
            return point

    class SerializedPooling(torch.nn.Module):
        def __init__(self, cin, cout, stride, norm_layer, act_layer, reduce, shuffle_orders, traceable=True):
            super().__init__()
            self.stride, self.reduce, self.shuffle_orders, self.traceable = stride, reduce, shuffle_orders, traceable
            self.proj = torch.nn.Linear(cin, cout)
            self.norm, self.act = PointSequential(norm_layer(cout)), PointSequential(act_layer())

        def forward(self, point):
            raise AssertionError("the module's own pooling ran for CUDA tensors")

    class SerializedUnpooling(torch.nn.Module):
        def __init__(self, cin, cskip, cout, norm_layer, act_layer, traceable=False):
            super().__init__()
            self.proj = PointSequential(torch.nn.Linear(cin, cout), norm_layer(cout), act_layer())
            self.proj_skip = PointSequential(torch.nn.Linear(cskip, cout), norm_layer(cout), act_layer())
            self.traceable = traceable

        def forward(self, point):
            parent, inverse = point.pop("pooling_parent"), point.pop("pooling_inverse")
            point, parent = self.proj(point), self.proj_skip(parent)
            parent.feat = parent.feat + point.feat[inverse]
            return parent

    return types.SimpleNamespace(Point=Point, SerializedPooling=SerializedPooling, SerializedUnpooling=SerializedUnpooling)


@pytest.fixture(scope="module")
def bound():
    M = _stand_in()
    PP.install(M)
    yield M
    PP.uninstall(M)


def _pair(dev, M, gold, case, shuffle=False, drop_plan=False, seed=None):
    bn = functools.partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    pool = M.SerializedPooling(20, 36, int(gold[case + ".stride"]), bn, torch.nn.GELU, str(gold[case + ".reduce"]), shuffle)
    unpool = M.SerializedUnpooling(36, 20, 12, bn, torch.nn.GELU)
    for name, module in (("pool", pool), ("unpool", unpool)):
        module.load_state_dict({k: torch.from_numpy(gold["w.%s.%s" % (name, k)]) for k in module.state_dict()})
        module.to(dev).train()
    if seed is not None:   # after the modules' own initialisation, which draws from the same generator
        torch.manual_seed(seed)
    g = lambda k: torch.from_numpy(gold["%s.int.%s" % (case, k)]).to(dev)  # noqa: E731
    feat = torch.from_numpy(gold["feat"]).to(dev).requires_grad_(True)
    point = M.Point(feat=feat, coord=torch.from_numpy(gold["coord"]).to(dev), grid_coord=torch.from_numpy(gold[case + ".grid"]).to(dev),
                    batch=torch.from_numpy(gold["batch"]).to(dev), grid_size=float(gold[case + ".grid_size"]),
                    serialized_code=g("in.serialized_code"), serialized_order=g("in.serialized_order"),
                    serialized_inverse=g("in.serialized_inverse"), serialized_depth=int(gold["%s.int.in.serialized_depth" % case]))
    pooled = pool(point)
    assert pooled["sparsified"] and pooled["pooling_parent"] is point and isinstance(pooled["pooling_plan"], PP.PoolPlan)
    ints = {k: pooled[k].cpu().numpy() for k in ("grid_coord", "serialized_code", "serialized_order", "serialized_inverse",
                                                 "batch", "pooling_inverse")}
    ints["serialized_depth"] = np.asarray(pooled["serialized_depth"])
    floats = {"feat": pooled.feat, "coord": pooled.coord}
    if drop_plan:
        del pooled["pooling_plan"]
    parent = unpool(pooled)
    assert parent is point and "pooling_plan" not in pooled and "pooling_parent" not in pooled
    floats["unpooled"] = parent.feat
    params = [("pool." + k, p) for k, p in pool.named_parameters()] + [("unpool." + k, p) for k, p in unpool.named_parameters()]
    grads = torch.autograd.grad((parent.feat * torch.from_numpy(gold["dout"]).to(dev)).sum(), [feat] + [p for _, p in params])
    floats["grad.feat"] = grads[0]
    for (name, _), gr in zip(params, grads[1:]):
        floats["grad." + name] = gr
    return ints, {k: v.detach().double().cpu().numpy() for k, v in floats.items()}


def _compare(gold, case, ints, floats):
    for k, v in ints.items():
        assert np.array_equal(v, gold["%s.int.%s" % (case, k)]), k
    worst = []
    for name, value in floats.items():
        want, err32 = gold["%s.%s" % (case, name)], float(gold["%s.err32.%s" % (case, name)])
        err = float(np.abs(value - want).max() / float(gold["%s.scale.%s" % (case, name)]))
        print("%s %-28s %.2e of the maximum, the reference's float32 run %.2e" % (case, name, err, err32))
        if not err <= 4 * err32:
            worst.append((name, err, err32))
    assert not worst, worst


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_rebound_modules_match_the_reference_run(cuda_device, bound, golden, case):
    PP.reset_stats()
    ints, floats = _pair(cuda_device, bound, golden, case)
    st = PP.stats()
    assert (st["pooling_fused"], st["unpooling_fused"], st["pooling_original"], st["unpooling_original"]) == (1, 1, 0, 0)
    assert st["plan_calls"] == 1 and st["reduce_calls"] == 2 and st["unpool_calls"] == 1 and st["reduce_backward_calls"] == 1
    assert set(floats) == {k[len(case) + 1:] for k in golden.files if k.startswith(case + ".") and k.split(".")[1] in
                           ("feat", "coord", "unpooled", "grad")}
    _compare(golden, case, ints, floats)


@pytest.mark.parametrize("case", ["a", "b"])
def test_unpooling_without_the_plan_takes_the_modules_own_path(cuda_device, bound, golden, case):
    PP.reset_stats()
    ints, floats = _pair(cuda_device, bound, golden, case, drop_plan=True)
    st = PP.stats()
    assert (st["pooling_fused"], st["unpooling_fused"], st["unpooling_original"], st["unpool_calls"]) == (1, 0, 1, 0)
    _compare(golden, case, ints, floats)


def test_shuffle_orders_is_one_draw_of_the_host_generator_in_the_same_place(cuda_device, bound, golden):
    seed = 4321
    ints, _ = _pair(cuda_device, bound, golden, "a", shuffle=True, seed=seed)
    after = torch.rand(1).item()
    torch.manual_seed(seed)
    perm = torch.randperm(3).numpy()
    assert torch.rand(1).item() == after   # the host generator advanced by exactly upstream's one draw
    for key in ("serialized_code", "serialized_order", "serialized_inverse"):
        assert np.array_equal(ints[key], golden["a.int." + key][perm]), key
    assert np.array_equal(ints["pooling_inverse"], golden["a.int.pooling_inverse"])
