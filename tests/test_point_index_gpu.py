"""-m gpu: the index plans of the point backbone on the device (gaussiancity_amd.point_index -> gcs_serialize /
gcs_patch_plan_* -> gfx950 kernels) against the numpy formulation in index_ref.py and the fixture recorded from
models/pt_v3.py on the CPU.  Integer work, and three correctly rounded binary32 operations for `cord`: the bar is
BIT-EXACT for every output."""
import os
import types

import numpy as np
import pytest
import torch

import index_ref as R
from gaussiancity_amd import point_index as PI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIX_BLOCK = 4096   # rows of one block of the sort's kernels: 256 threads x 16 keys
SCAN_MIN_BLOCKS = 256   # blocks up to which a pass of the sort is two launches (gcs_index.h)
SIZES = (1, 63, 64, 65, 255, 256, 257, RADIX_BLOCK - 1, RADIX_BLOCK, RADIX_BLOCK + 1, 100_003)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ptv3_index.npz"))


def _run(dev, grid, batch, depth, orders, grid_size=0.01, n_batches=1):
    g = torch.from_numpy(np.ascontiguousarray(grid)).to(dev)
    b = None if batch is None else torch.from_numpy(batch).to(dev)
    out = PI.serialize(g, b, depth, orders, grid_size, n_batches)
    assert all(t.dtype == torch.int64 and tuple(t.shape) == (len(orders), len(grid)) and t.device == g.device for t in out)
    return out


def _check(dev, grid, batch, depth, orders, grid_size=0.01, n_batches=1, what=""):
    """Library against index_ref, against torch's stable sort on the device, and inverse against order."""
    code, order, inverse = _run(dev, grid, batch, depth, orders, grid_size, n_batches)
    want = R.serialize(grid, batch, depth, orders, grid_size)
    for got, ref, key in zip((code, order, inverse), want, ("code", "order", "inverse")):
        g = got.cpu().numpy()
        for r, name in enumerate(orders):
            assert np.array_equal(g[r], ref[r]), (what, key, name)
    assert torch.equal(order, torch.sort(code, dim=1, stable=True).indices)
    n = len(grid)
    assert torch.equal(torch.gather(inverse, 1, order), torch.arange(n, device=dev).expand(len(orders), n))
    return code, order, inverse


def _points(rng, n, depth, n_batches):
    grid = rng.integers(0, 1 << depth, (n, 3)).astype(np.int32)
    grid[n // 2] = grid[0]   # two rows on one voxel: a tie within a batch at least when they share the batch
    batch = rng.integers(0, n_batches, n).astype(np.int64)
    batch[n // 2] = batch[0]
    return grid, batch


@pytest.mark.parametrize("n", SIZES)
def test_all_five_orders_at_every_size(cuda_device, n):
    grid, batch = _points(np.random.default_rng(n), n, 8, 57)
    _check(cuda_device, grid, batch, 8, R.ORDERS, n_batches=57)


def test_more_blocks_than_a_scatter_block_sums_itself(cuda_device):
    """Up to 256 blocks of rows the scatter sums the per-block digit counts itself; one row more takes the scan kernel."""
    for n in (SCAN_MIN_BLOCKS * RADIX_BLOCK, SCAN_MIN_BLOCKS * RADIX_BLOCK + 1):
        grid, batch = _points(np.random.default_rng(n), n, 8, 57)
        _check(cuda_device, grid, batch, 8, ("cord", "z"), n_batches=57)


@pytest.mark.parametrize("depth,n_batches", [(1, 3), (8, 57), (11, 57), (16, 127), (16, 32767)])
def test_depths_and_batch_bits(cuda_device, depth, n_batches):
    """depth 11 with 57 batches: the batch bits cross bit 32; depth 16 with 32767 batches: bit 62, the last one."""
    rng = np.random.default_rng(depth * 100003 + n_batches)
    grid, batch = _points(rng, 1000, depth, n_batches)
    batch[1] = n_batches - 1
    grid[2] = (1 << depth) - 1
    code, _, _ = _check(cuda_device, grid, batch, depth, R.ORDERS, n_batches=n_batches)
    curves = code[1:]
    assert int(curves.max()).bit_length() == 3 * depth + (n_batches - 1).bit_length()
    _check(cuda_device, grid, None, depth, R.ORDERS, what="batch=None")


@pytest.mark.parametrize("name", R.ORDERS)
def test_each_order_alone(cuda_device, name):
    grid, batch = _points(np.random.default_rng(11), RADIX_BLOCK + 1, 8, 57)
    _check(cuda_device, grid, batch, 8, (name,), n_batches=57)


def test_coordinates_are_taken_modulo_the_cube_and_cord_as_they_are(cuda_device):
    """Coordinates above 2^depth and negative ones: the curve orders mask them, `cord` sorts negative codes first."""
    rng = np.random.default_rng(5)
    grid = rng.integers(-300, 3000, (777, 3)).astype(np.int32)
    code, order, _ = _check(cuda_device, grid, None, 8, R.ORDERS)
    assert int(code[0].min()) < 0 and int(code[0, order[0, 0]]) == int(code[0].min())
    assert int(code[1:].min()) >= 0 and int(code[1:].max()) < 1 << 24


def test_equal_codes_keep_their_rows_in_place(cuda_device):
    """Stability: every code equal (and no digit differs, so every pass is skippable): order = inverse = arange."""
    n = RADIX_BLOCK + 904
    grid = np.tile(np.array([[3, 200, 77]], np.int32), (n, 1))
    code, order, inverse = _check(cuda_device, grid, np.full(n, 4, np.int64), 8, R.ORDERS, n_batches=57)
    assert bool((code == code[:, :1]).all())
    ar = torch.arange(n, device=cuda_device).expand(5, n)
    assert torch.equal(order, ar) and torch.equal(inverse, ar)


def test_ties_fall_to_the_lower_row(cuda_device):
    """The `cord` collision of (x, 1, 0) and (x, 0, 100) at grid_size 0.01, many times over, in runs across blocks."""
    n = 3 * RADIX_BLOCK + 17
    rng = np.random.default_rng(3)
    x = rng.integers(0, 6, n)
    flip = rng.integers(0, 2, n)
    grid = np.stack([x, flip, 100 * (1 - flip)], 1).astype(np.int32)
    code, order, _ = _check(cuda_device, grid, None, 8, ("cord",))
    assert len(np.unique(code.cpu().numpy())) == 6
    o = order[0].cpu().numpy()
    same = np.diff(code[0].cpu().numpy()[o]) == 0
    assert bool((np.diff(o)[same] > 0).all()) and int(same.sum()) == n - 6


def test_codes_that_differ_only_above_bit_40(cuda_device):
    """The five low byte digits are constant over all keys: those passes are skipped, the result is the same sort."""
    rng = np.random.default_rng(9)
    grid = (rng.integers(0, 4, (RADIX_BLOCK + 5, 3)) << 14).astype(np.int32)
    code, _, _ = _check(cuda_device, grid, None, 16, ("z", "z-trans", "hilbert", "hilbert-trans"))
    z = code[:2].cpu().numpy()
    assert not (z & ((1 << 40) - 1)).any() and len(np.unique(z[0])) == 64


@pytest.mark.parametrize("depth", (1, 5, 8, 11, 16))
def test_golden_codes_on_the_device(cuda_device, golden, depth):
    grid, batch = golden["d%d.grid" % depth], golden["d%d.batch" % depth]
    for with_batch in (0, 1):
        code, _, _ = _check(cuda_device, grid, batch if with_batch else None, depth, R.ORDERS, n_batches=5)
        assert np.array_equal(code.cpu().numpy(), golden["d%d.code.%d" % (depth, with_batch)]), with_batch


def test_golden_cord_division_on_the_device(cuda_device, golden):
    code, _, _ = _check(cuda_device, golden["cord003.grid"], None, 9, ("cord",), grid_size=0.003)
    assert np.array_equal(code.cpu().numpy(), golden["cord003.code"])
    code, _, _ = _check(cuda_device, golden["cord256.grid"], None, 8, ("cord",), grid_size=0.01)
    assert np.array_equal(code.cpu().numpy(), golden["cord256.code"])


def test_cord_against_torch_on_the_device(cuda_device, capsys):
    """The library's `cord` is pinned to the division (index_ref, the golden).  How many elements torch's own on-device
    evaluation of the expression gives differently is REPORTED, not asserted: its kernel may multiply by the reciprocal."""
    a = np.arange(256, dtype=np.int32)
    grid = np.stack(np.meshgrid(a, a, np.array([0, 7, 255], np.int32), indexing="ij"), -1).reshape(-1, 3)
    code, _, _ = _check(cuda_device, grid, None, 8, ("cord",))
    g = torch.from_numpy(grid).to(cuda_device).long()
    theirs = (g[:, 0] / 0.01 ** 2 + g[:, 1] / 0.01 + g[:, 2]).long()
    differing = int((theirs != code[0]).sum())
    with capsys.disabled():
        print("\ncord, coordinates below 256 at grid_size 0.01: torch on the device differs from the division in %d of %d "
              "elements" % (differing, len(grid)))


def _plan(dev, counts, patch):
    offset = torch.from_numpy(np.cumsum(counts).astype(np.int64)).to(dev)
    pad, unpad, cu = PI.patch_plan(offset, patch)
    assert (pad.dtype, unpad.dtype, cu.dtype) == (torch.int64, torch.int64, torch.int32)
    assert pad.device == unpad.device == cu.device == offset.device
    return pad.cpu().numpy(), unpad.cpu().numpy(), cu.cpu().numpy()


@pytest.mark.parametrize("name", ("p4", "p1024", "p16", "p32", "one", "zero"))
def test_golden_patch_plans_on_the_device(cuda_device, golden, name):
    got = _plan(cuda_device, golden[name + ".counts"], int(golden[name + ".patch"]))
    for g, key in zip(got, ("pad", "unpad", "cu")):
        want = golden["%s.%s" % (name, key)]
        assert g.dtype == want.dtype and np.array_equal(g, want), key


def test_patch_plan_of_a_frame(cuda_device):
    """57 batches of 1...5000 rows at patch 1024 (an inference frame's shape), and one long batch cut into row slices."""
    counts = np.random.default_rng(57).integers(1, 5001, 57)
    for c, patch in ((counts, 1024), (np.array([150_001]), 1024), (np.array([150_001, 3]), 7)):
        got = _plan(cuda_device, c, patch)
        for g, want in zip(got, R.patch_plan(np.cumsum(c), patch)):
            assert g.dtype == want.dtype and np.array_equal(g, want)


class _Dict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _stand_in():
    class Point(_Dict):
        def serialization(self, order="z", depth=None, shuffle_orders=False):
            raise AssertionError("the original method ran for CUDA tensors")

    class SerializedAttention:
        patch_size = 64

        def get_padding_and_inverse(self, point):
            raise AssertionError("the original method ran for CUDA tensors")

    return types.SimpleNamespace(Point=Point, SerializedAttention=SerializedAttention)


def test_install_runs_the_library_and_reuses_the_cached_keys(cuda_device):
    M = _stand_in()
    PI.install(M)
    try:
        PI.reset_stats()
        counts = np.array([100, 7, 300, 64, 65])
        n = int(counts.sum())
        rng = np.random.default_rng(1)
        coord = rng.uniform(-1.0, 1.5, (n, 3)).astype(np.float32)
        batch = np.repeat(np.arange(5), counts)
        point = M.Point(coord=torch.from_numpy(coord).to(cuda_device), grid_size=0.01,
                        batch=torch.from_numpy(batch).to(cuda_device),
                        offset=torch.from_numpy(np.cumsum(counts)).to(cuda_device))
        names = ["z", "cord", "hilbert", "z"]   # a repeated order, as upstream allows
        torch.manual_seed(1234)
        point.serialization(order=names, shuffle_orders=True)
        after = torch.rand(1).item()
        torch.manual_seed(1234)
        perm = torch.randperm(len(names)).tolist()
        assert torch.rand(1).item() == after   # the host generator advanced by exactly upstream's one draw
        grid = point["grid_coord"]
        assert grid.dtype == torch.int32 and grid.is_cuda
        c = point["coord"]
        want_grid = torch.div(c - c.min(0)[0], 0.01, rounding_mode="trunc").int().cpu()   # derived by torch, as upstream
        assert torch.equal(grid.cpu(), want_grid)
        depth = int(want_grid.max()).bit_length()
        assert point["serialized_depth"] == depth == 8
        want = R.serialize(want_grid.numpy(), batch, depth, [names[i] for i in perm], 0.01)
        for key, ref in zip(("serialized_code", "serialized_order", "serialized_inverse"), want):
            assert np.array_equal(point[key].cpu().numpy(), ref), key
        assert PI.stats() == {"serialize_calls": 1, "patch_plan_calls": 0}
        att = M.SerializedAttention()
        first = att.get_padding_and_inverse(point)
        second = att.get_padding_and_inverse(point)
        assert PI.stats() == {"serialize_calls": 1, "patch_plan_calls": 1}
        assert all(a is b for a, b in zip(first, second)) and first[0] is point["pad"] and first[2] is point["cu_seqlens_key"]
        for g, ref in zip(first, R.patch_plan(np.cumsum(counts), 64)):
            assert np.array_equal(g.cpu().numpy(), ref) and g.cpu().numpy().dtype == ref.dtype
    finally:
        PI.uninstall(M)
