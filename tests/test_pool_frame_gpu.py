"""The pooling plan and the gathered reduce at the sizes where a frame takes them (gaussiancity_amd/csrc/gcs_pool.h,
DESIGN.md section 15.6): plans of more than two tiles and of more than 256, with heads placed on the edges of tiles and of
a thread's sixteen positions; the plan through the C ABI into the test's own guarded buffers; and reduces with more work
items than one grid covers, so that the kernels' stride loops run a second and a third time.

Every comparison is on bits, and none is with this library's own segment_csr: the plans against pool_ref.plan_fast, the
reduce, its transpose and the expanding add against pool_ref.gather_reduce / gather_backward / expand_add, which are the
contract of include/gcs.h in numpy's float32.  There is no tolerance in this file.  tests/test_pool_ref_host.py holds the
references and the cases (tests/pool_cases.py) to what they promise, without a GPU."""
import functools

import numpy as np
import pytest
import torch

import pool_cases as K
import pool_ref as R
from gaussiancity_amd import _native_s as S
from gaussiancity_amd import point_pool as PP
from test_point_pool_gpu import DTYPES, REDUCES, SEGMENTS, WIDTHS, _codes, _hand_plan, _source

pytestmark = pytest.mark.gpu
PLAN_FIELDS = ("cluster", "indices", "idx_ptr", "head", "code", "order", "inverse")


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(t, want):
    """A device tensor and a numpy array hold the same bits (dtype and shape included)."""
    got = t.detach().cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


# ---------------------------------------------------------------------------------------------- the plan
def _check_plan(dev, code, shift):
    plan = PP.pool_plan(torch.from_numpy(code).to(dev), shift // 3)
    want = R.plan_fast(code, shift)
    assert (plan.n, plan.s) == (want.n, want.s)
    for name in PLAN_FIELDS:
        got = getattr(plan, name)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), getattr(want, name)), name
    return want


@pytest.mark.parametrize("shift", [0, 3, 9])
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("n", K.PLAN_TILE_SIZES)
def test_plan_of_more_than_two_tiles(cuda_device, n, k, shift):
    """k_pool_emit's tile prefix is a sum of several counts from the third tile on."""
    rng = np.random.default_rng(1000 * n + 10 * k + shift)
    for pattern in ("mixed", "one", "distinct", "batch"):
        _check_plan(cuda_device, _codes(rng, pattern, n, k, shift), shift)


@pytest.mark.parametrize("k,shift", [(1, 0), (3, 3)])
@pytest.mark.parametrize("name", list(K.placed_cases()))
def test_plan_with_heads_placed_on_purpose(cuda_device, name, k, shift):
    """Heads on both sides of every tile edge and of every thread's sixteen positions; tiles without a head in front of a
    tile that is all heads; one cluster; n clusters."""
    n, heads = K.placed_cases()[name]
    want = _check_plan(cuda_device, K.placed_codes(K.sizes_for_heads(n, heads), k, shift, seed=len(name)), shift)
    assert want.idx_ptr[:-1].tolist() == sorted(set([0] + list(heads)))


@pytest.mark.parametrize("pattern,k,shift", K.ROUNDS_CASES)
def test_plan_of_more_than_256_tiles(cuda_device, pattern, k, shift):
    """257 tiles: k_pool_total's second round and the sort's scan kernel in _count; with every key its own cluster, the
    scan kernel in _emit's sort of the pooled rows too, on its own layout inside the same workspace."""
    want = _check_plan(cuda_device, _codes(np.random.default_rng(k), pattern, K.N_ROUNDS, k, shift), shift)
    assert (want.s == 1) if pattern == "one" else (want.s == K.N_ROUNDS) if pattern == "distinct" else (1000 < want.s < want.n)


GUARD_BYTES, GUARD_WORDS = 4096, 512
SENTINEL, WS_GUARD, OUT_GUARD = -7, 0xA5, 0x5A5A5A5A5A5A5A5A


def _raw_plan(dev, code, shift, fill):
    """gcs_pool_plan_count and _emit with the test's own buffers: the workspace filled with `fill` and followed by guard
    bytes, every output sized exactly, filled with a sentinel and followed by guard words.  Returns (s, outputs) after
    asserting that no guard changed."""
    L = S.lib()
    k, n = code.shape
    need = L.gcs_pool_plan_workspace_bytes(n, k)
    assert need > 0
    ws = torch.full((need + GUARD_BYTES,), WS_GUARD, dtype=torch.uint8, device=dev)
    ws[:need] = fill
    c = torch.from_numpy(code).to(dev)
    count = torch.full((1,), SENTINEL, dtype=torch.int64).pin_memory()
    torch.cuda.synchronize()
    S.check(L.gcs_pool_plan_count(c.data_ptr(), k, n, shift, ws.data_ptr(), need, count.data_ptr(), None), "gcs_pool_plan_count")
    s = int(count[0])
    assert 1 <= s <= n
    sizes = (n, n, s + 1, s, k * s, k * s, k * s)
    bufs = []
    for size in sizes:
        b = torch.full((size + GUARD_WORDS,), SENTINEL, dtype=torch.int64, device=dev)
        b[size:] = OUT_GUARD
        bufs.append(b)
    S.check(L.gcs_pool_plan_emit(c.data_ptr(), k, n, shift, s, ws.data_ptr(), need, *[b.data_ptr() for b in bufs], None),
            "gcs_pool_plan_emit")
    torch.cuda.synchronize()
    assert bool((ws[need:] == WS_GUARD).all()), "a store behind the workspace"
    for name, b, size in zip(PLAN_FIELDS, bufs, sizes):
        assert bool((b[size:] == OUT_GUARD).all()), "a store behind " + name
    return s, [b[:size].cpu().numpy() for b, size in zip(bufs, sizes)]


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("n", [K.N_PLACED, K.N_ROUNDS])
def test_plan_through_the_abi_keeps_to_its_buffers(cuda_device, n, k):
    """Every output is written entirely (no sentinel is left: it equals the reference) and nothing behind it or behind the
    workspace is; what the workspace held before the call, zeros or ones, does not reach the outputs."""
    shift = 3
    pattern = "mixed" if n == K.N_PLACED else "distinct"   # distinct: s = n, the largest outputs the sizes allow
    code = _codes(np.random.default_rng(n + k), pattern, n, k, shift)
    want = R.plan_fast(code, shift)
    for fill in (0x00, 0xFF):
        s, outs = _raw_plan(cuda_device, code, shift, fill)
        assert s == want.s
        for name, got in zip(PLAN_FIELDS, outs):
            assert np.array_equal(got, getattr(want, name).reshape(-1)), (name, fill)


# ---------------------------------------------------------------------------------------------- past the grid cap
def _device_plan(dev, hp):
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    z = torch.zeros((1, hp.s), dtype=torch.int64, device=dev)
    return PP.PoolPlan(t(hp.cluster), t(hp.indices), t(hp.idx_ptr), t(hp.head), z, z, z, hp.n, hp.s)


@functools.lru_cache(maxsize=2)
def _grid_case(name):
    """(host plan, source with ties, source without, dout, parent, child) of a case, shared by its tests and left as it is."""
    f, dtype, _, _ = K.GRID_CASES[name]
    hp = K.grid_plan(name)
    seed = 10 * list(K.GRID_CASES).index(name)
    return (hp, K.values((hp.n, f), dtype, seed + 1, True), K.values((hp.n, f), dtype, seed + 2, False),
            K.values((hp.s, f), dtype, seed + 3, False), K.values((hp.n, f), dtype, seed + 4, False),
            K.values((hp.s, f), dtype, seed + 5, False))


def _reduce_case(dev, hp, x_host, dout_host, reduce, view=None):
    """Forward, backward through autograd, and the backward into a NaN-filled buffer, each twice, against the reference.
    `view` turns the device copy of the source into the tensor that is reduced (a column slice)."""
    plan = _device_plan(dev, hp)
    want, want_arg = R.gather_reduce(x_host, hp.indices, hp.idx_ptr, reduce)
    want_grad = R.gather_backward(dout_host, hp.cluster, hp.idx_ptr, reduce, want_arg)
    dout = torch.from_numpy(dout_host).to(dev)
    for _ in range(2):   # run to run
        x = torch.from_numpy(x_host).to(dev) if view is None else view(dev)
        assert _same(x, x_host)
        out, arg = PP.gather_forward(x, plan, reduce)
        assert _same(out, want), reduce
        assert (arg is None and want_arg is None) or _same(arg, want_arg), reduce
        leaf = x.detach().requires_grad_(True)
        res = PP.pooled_reduce(leaf, plan, reduce)
        assert _same(res, want), reduce
        res.backward(dout)
        assert _same(leaf.grad, want_grad), reduce
        buf = torch.full((hp.n, x_host.shape[1]), float("nan"), dtype=dout.dtype, device=dev)
        assert PP.gather_backward(dout, plan, reduce, arg, out=buf) is buf and _same(buf, want_grad), reduce
    return want_arg, want_grad


@pytest.mark.parametrize("name,reduce", [(name, r) for name, case in K.GRID_CASES.items() for r in case[3]])
def test_reduce_past_the_grid_cap(cuda_device, name, reduce):
    """More than 2.3 grids of work items, forward and backward: what a thread carries from one trip of its stride loop
    into the next (res, best, acc, the segment's bounds) shows in the second and third trip only."""
    hp, ties, plain, dout = _grid_case(name)[:4]
    assert min(K.item_counts(name, hp)) > 2 * K.GRID_CAP
    _reduce_case(cuda_device, hp, ties if reduce in ("min", "max") else plain, dout, reduce)


@pytest.mark.parametrize("name", list(K.GRID_CASES))
def test_unpool_add_past_the_grid_cap(cuda_device, name):
    """unpool_add forward (one fp32 add, rounded once) and backward (d_parent is dout, d_child its gathered sum)."""
    hp, _, up_host, _, a_host, b_host = _grid_case(name)
    plan = _device_plan(cuda_device, hp)
    want = R.expand_add(a_host, b_host, hp.cluster)
    want_child, _ = R.gather_reduce(up_host, hp.indices, hp.idx_ptr, "sum")
    up = torch.from_numpy(up_host).to(cuda_device)
    for _ in range(2):
        a = torch.from_numpy(a_host).to(cuda_device).requires_grad_(True)
        b = torch.from_numpy(b_host).to(cuda_device).requires_grad_(True)
        out = PP.unpool_add(a, b, plan)
        assert _same(out, want)
        out.backward(up)
        assert _same(a.grad, up_host) and _same(b.grad, want_child)
        assert _same(PP.unpool_add(None, b.detach(), plan), b_host[hp.cluster])


@functools.lru_cache(maxsize=1)
def _wide_source(name):
    f, dtype, _, _ = K.GRID_CASES[name]
    return K.values((K.grid_plan(name).n, f + 8), dtype, 77, True)


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("start", ["aligned", 1])
@pytest.mark.parametrize("name", ["wide_f32", "wide_f16"])
def test_reduce_of_a_column_slice_past_the_grid_cap(cuda_device, name, start, reduce):
    """The source as a column slice of a wider tensor, read in place: from a column that keeps the rows 16-byte aligned
    (16-byte pieces, row stride f + 8), and from column 1 (one element at a time at f = 512, four or eight times the
    items).  The backward writes a slice of a NaN-filled wider buffer and leaves the columns around it alone."""
    f, dtype, _, _ = K.GRID_CASES[name]
    hp, _, _, dout_host = _grid_case(name)[:4]
    first = 1 if start == 1 else 16 // np.dtype(dtype).itemsize
    wide_host = _wide_source(name)
    x_host = np.ascontiguousarray(wide_host[:, first:first + f])

    def view(dev):
        v = torch.from_numpy(wide_host).to(dev)[:, first:first + f]
        assert not v.is_contiguous() and (v.data_ptr() % 16 == 0) == (start == "aligned")
        return v

    want_arg, want_grad = _reduce_case(cuda_device, hp, x_host, dout_host, reduce, view=view)
    arg = None if want_arg is None else torch.from_numpy(want_arg).to(cuda_device)
    buf = torch.full((hp.n, f + 8), float("nan"), dtype=DTYPES[dtype], device=cuda_device)
    PP.gather_backward(torch.from_numpy(dout_host).to(cuda_device), _device_plan(cuda_device, hp), reduce, arg,
                       out=buf[:, first:first + f])
    assert _same(buf[:, first:first + f].contiguous(), want_grad)
    assert bool(torch.isnan(buf[:, :first]).all()) and bool(torch.isnan(buf[:, first + f:]).all())


# ---------------------------------------------------------------------------------------------- the small shapes again
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_small_shapes_against_the_independent_reference(cuda_device, dtype, f):
    """The shapes of test_point_pool_gpu's forward and backward tests, with and without ties, held to the contract's bits
    instead of to segment_csr: forward and arg, the backward, the expanding add and its backward."""
    dt = DTYPES[dtype]
    host = lambda t: t.detach().cpu().numpy()  # noqa: E731
    for s in SEGMENTS:
        plan = _hand_plan(cuda_device, s, 300 * f + s)
        indices, idx_ptr, cluster = host(plan.indices), host(plan.idx_ptr), host(plan.cluster)
        g = torch.Generator().manual_seed(s)
        dout = torch.randn(plan.s, f, generator=g).to(dt).to(cuda_device)
        for ties in (False, True):
            x = _source(cuda_device, plan.n, f, dt, 2 * f + s, ties)
            for reduce in REDUCES:
                want, want_arg = R.gather_reduce(host(x), indices, idx_ptr, reduce)
                out, arg = PP.gather_forward(x, plan, reduce)
                assert _same(out, want), (s, reduce, ties)
                assert (arg is None and want_arg is None) or _same(arg, want_arg), (s, reduce, ties)
                leaf = x.clone().requires_grad_(True)
                PP.pooled_reduce(leaf, plan, reduce).backward(dout)
                assert _same(leaf.grad, R.gather_backward(host(dout), cluster, idx_ptr, reduce, want_arg)), (s, reduce, ties)
        a = _source(cuda_device, plan.n, f, dt, 5, False).requires_grad_(True)
        b = _source(cuda_device, plan.s, f, dt, 6, False).requires_grad_(True)
        up = torch.randn(plan.n, f, generator=g).to(dt).to(cuda_device)
        out = PP.unpool_add(a, b, plan)
        assert _same(out, R.expand_add(host(a), host(b), cluster)), s
        out.backward(up)
        assert _same(a.grad, host(up)) and _same(b.grad, R.gather_reduce(host(up), indices, idx_ptr, "sum")[0]), s
