"""-m gpu: the device-resident volume path of libgcv_hip.so through its C ABI -- gcv_points_bounds, gcv_rows_to_volume,
gcv_rows_erase_volume and the occupancy bitmask -- against the numpy reference tests/rows_ref.py on its CASES (which
tests/test_rows_volume_host.py ties to the kernel paths they are named for), then points.visible_point_map on rows that
the extruder would never write.  Integer work: the bar is equality, voxel for voxel and bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import points_util as U
import rows_ref as R
from gaussiancity_amd import _native_v as V
from gaussiancity_amd import points as P
from gaussiancity_amd._loader import current_stream as _stream

pytestmark = pytest.mark.gpu

GUARD = 64                        # canary words in front of and behind every buffer a kernel writes
CANARY = 0x3c3c3c3c
STALE = 0x7f7f7f7f                # what the buffers hold before a call: above every id, every bit but one per byte
NAMES = list(R.CASES)


@pytest.fixture(scope="module")
def po():
    from oracle import points_oracle as PO
    PO.lib()
    return PO


class Guarded:
    """An int32 device buffer of n words between two runs of canary words."""

    def __init__(self, n, dev, fill=STALE):
        self.all = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int32, device=dev)
        self.body = self.all[GUARD:GUARD + n]
        self.body.fill_(fill)
        self.ptr = self.all.data_ptr() + 4 * GUARD

    def intact(self):
        return bool((self.all[:GUARD] == CANARY).all()) and bool((self.all[GUARD + self.body.numel():] == CANARY).all())


def _to(dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)   # (a copy: the references are read-only)


@functools.lru_cache(maxsize=None)
def _case_on(dev, name):
    """(rows on the device, offset[3], h, w, d, reference volume on the device, reference occupancy bytes)."""
    rows, offset, h, w, d = R.case(name)
    vol, occ = R.reference(name)
    return _to(dev, rows), (C.c_int32 * 3)(*offset), h, w, d, _to(dev, vol), occ


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _rows_to_volume(rows, off, h, w, d, volume_ptr, occ_ptr, volume_is_zero):
    V.check(V.lib().gcv_rows_to_volume(int(rows.shape[0]), _ptr(rows), off, h, w, d, volume_ptr, occ_ptr,
                                       volume_is_zero, _stream()), "gcv_rows_to_volume")


def _occ_bytes(g):
    return g.body.cpu().numpy().view(np.uint8)


def _same_bits(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d of %d bytes differ, first at byte %d: %#x for %#x" % (
        what, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])


def _same_volume(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        k, j, l = (int(v) for v in bad[0])
        raise AssertionError("%s: %d voxels differ, first at (y, x, z) = (%d, %d, %d): %d for %d" % (
            what, bad.shape[0], k, j, l, int(got[k, j, l]), int(want[k, j, l])))


# ---- 1. volume and occupancy, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_rows_to_volume_and_occupancy(cuda_device, name):
    rows, off, h, w, d, want, want_occ = _case_on(cuda_device, name)
    lib = V.lib()
    assert lib.gcv_occupancy_bytes(h, w, d) == want_occ.size
    vol, occ = Guarded(h * w * d, cuda_device), Guarded(want_occ.size // 4, cuda_device)
    for run in range(2):   # stale contents in front of both runs: the second sees the first's result as well
        if run:
            vol.body.bitwise_xor_(0x55555555)
            occ.body.fill_(-1)
        _rows_to_volume(rows, off, h, w, d, vol.ptr, occ.ptr, 0)
        _same_volume(vol.body.view(h, w, d), want, "run %d" % run)
        _same_bits(_occ_bytes(occ), want_occ, "occupancy, run %d" % run)
        assert vol.intact() and occ.intact()
    # the bitmask that gcv_build_occupancy makes of that volume
    occ2 = Guarded(want_occ.size // 4, cuda_device)
    V.check(lib.gcv_build_occupancy(vol.ptr, h, w, d, occ2.ptr, _stream()), "gcv_build_occupancy")
    _same_bits(_occ_bytes(occ2), want_occ, "gcv_build_occupancy")
    assert occ2.intact()


# ---- 2. gcv_points_to_volume: its own copy of the straddle loops, explicit ids, a scale per axis ----------------------
@pytest.mark.parametrize("name", ["big_cubes", "faces", "many_words"])
def test_points_to_volume_on_the_same_geometry(cuda_device, name):
    rows, offset, h, w, d = R.case(name)
    n = len(rows)
    rng = np.random.default_rng(17)
    pts = R.localize(rows, offset)
    ids = (rng.permutation(n) * 5 + 2).astype(np.int32)        # distinct, in no order: the highest id wins, not the last row
    sc = np.repeat(rows[:, 3:4], 3, axis=1)
    k = np.arange(0, n, 3)
    sc[k, k % 3] = np.maximum(1, sc[k, k % 3] - 1 - k % 5)     # every third row is no cube
    want = R.reference_points_volume(pts, ids, sc, h, w, d)
    want_occ = R.reference_occupancy(want)
    t = [_to(cuda_device, a) for a in (pts, ids, sc)]
    want_d = _to(cuda_device, want)
    vol, occ = Guarded(h * w * d, cuda_device), Guarded(want_occ.size // 4, cuda_device)
    for run in range(2):
        V.check(V.lib().gcv_points_to_volume(n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), h, w, d, vol.ptr,
                                             occ.ptr, _stream()), "gcv_points_to_volume")
        _same_volume(vol.body.view(h, w, d), want_d, "run %d" % run)
        _same_bits(_occ_bytes(occ), want_occ, "occupancy, run %d" % run)
        assert vol.intact() and occ.intact()
    if name == "big_cubes":   # with the case's own cubes and ids it is gcv_rows_to_volume's result
        t[1] = _to(cuda_device, np.arange(1, n + 1, dtype=np.int32))
        t[2] = _to(cuda_device, np.repeat(rows[:, 3:4], 3, axis=1))
        V.check(V.lib().gcv_points_to_volume(n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), h, w, d, vol.ptr,
                                             occ.ptr, _stream()), "gcv_points_to_volume")
        _same_volume(vol.body.view(h, w, d), _case_on(cuda_device, name)[5], "cubes")
        _same_bits(_occ_bytes(occ), R.reference(name)[1], "occupancy, cubes")


# ---- 3. volume_is_zero = 1 on a zero buffer --------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_rows_to_volume_into_a_zero_buffer(cuda_device, name):
    rows, off, h, w, d, want, want_occ = _case_on(cuda_device, name)
    vol, occ = Guarded(h * w * d, cuda_device, fill=0), Guarded(want_occ.size // 4, cuda_device)
    _rows_to_volume(rows, off, h, w, d, vol.ptr, occ.ptr, 1)
    _same_volume(vol.body.view(h, w, d), want, "volume_is_zero")
    _same_bits(_occ_bytes(occ), want_occ, "occupancy")
    assert vol.intact() and occ.intact()


# ---- 4. the erase is exact -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_erase_clears_the_written_voxels_and_no_other(cuda_device, name):
    rows, off, h, w, d, want, _ = _case_on(cuda_device, name)
    vol = Guarded(h * w * d, cuda_device)
    _rows_to_volume(rows, off, h, w, d, vol.ptr, None, 0)      # without a bitmask
    body = vol.body.view(h, w, d)
    _same_volume(body, want, "no occupancy")
    sentinel = torch.full_like(want, -7)
    body.copy_(torch.where(want == 0, sentinel, body))         # every voxel no cube owns
    V.check(V.lib().gcv_rows_erase_volume(int(rows.shape[0]), _ptr(rows), off, h, w, d, vol.ptr, _stream()),
            "gcv_rows_erase_volume")
    _same_volume(body, torch.where(want == 0, sentinel, torch.zeros_like(want)), "after the erase")
    assert vol.intact()


# ---- 5. bounds -------------------------------------------------------------------------------------------------------
def _bounds(dev, table, stride):
    """gcv_points_bounds of an int16 [n, stride] table, with garbage in the scratch."""
    lib = V.lib()
    words = lib.gcv_bounds_scratch_bytes() // 4
    garbage = np.random.default_rng(5).integers(-2 ** 31, 2 ** 31, words).astype(np.int32)
    garbage[::2] = np.where(np.arange(0, words, 2) % 4 == 0, -2 ** 31, 2 ** 31 - 1)   # beyond every int16, both ways
    scratch = _to(dev, garbage)
    t = _to(dev, table)
    assert t.shape[1] == stride
    mn, mx = (C.c_int32 * 3)(7, 7, 7), (C.c_int32 * 3)(-7, -7, -7)
    V.check(lib.gcv_points_bounds(int(t.shape[0]), t.data_ptr(), stride, scratch.data_ptr(), mn, mx, _stream()),
            "gcv_points_bounds")
    return [list(mn), list(mx)]


def _check_bounds(dev, rows):
    """Strides 5, 3 and 4; the columns behind the third hold values beyond every coordinate."""
    want = [v.tolist() for v in R.reference_bounds(rows)]
    n = len(rows)
    for stride in (5, 3, 4):
        table = np.empty((n, stride), np.int16)
        table[:, :3] = rows[:, :3]
        table[:, 3:] = np.where(np.arange(n)[:, None] % 2 == 0, -32768, 32767)
        assert _bounds(dev, table, stride) == want, (n, stride)


@pytest.mark.parametrize("name", [n for n in NAMES if n != "ragged_0"])
def test_bounds_of_every_case(cuda_device, name):
    _check_bounds(cuda_device, R.case(name)[0])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_bounds_of_partial_waves_and_blocks(cuda_device, n):
    rng = np.random.default_rng(400 + n)
    rows = rng.integers(-32768, 32768, (n, 5)).astype(np.int16)
    _check_bounds(cuda_device, rows)
    for last in (-32768, 32767):      # the extremum of every axis in the last row alone
        rows = rng.integers(-32000, 32000, (n, 5)).astype(np.int16)
        rows[n - 1, :3] = last
        _check_bounds(cuda_device, rows)


def test_bounds_of_planted_extrema_beyond_one_grid_pass(cuda_device):
    """1024 blocks x 256 threads cover 262 144 rows in one pass; 300 more make a second.  Six extrema, one row each."""
    one_pass = 1024 * 256
    n = one_pass + 300
    rows = np.random.default_rng(6).integers(-1000, 1001, (n, 5)).astype(np.int16)
    planted = {"min x": (0, 0, -32768),                        # the very first row
               "max x": (n - 1, 0, 32767),                     # the very last row
               "min y": (one_pass + 150, 1, -20000),           # a row of the second pass
               "max y": (256 * 500 + 255, 1, 20000),           # the last lane of a block's last wave
               "min z": (256 * 1023, 2, -32767),               # the first row of the last block
               "max z": (one_pass, 2, 32766)}                  # the first row of the second pass
    for row, col, value in planted.values():
        rows[row, col] = value
    mn, mx = R.reference_bounds(rows)
    assert mn.tolist() == [-32768, -20000, -32767] and mx.tolist() == [32767, 20000, 32766]
    _check_bounds(cuda_device, rows)


# ---- 6. through the wrapper ------------------------------------------------------------------------------------------
def test_visible_point_map_on_adversarial_rows(cuda_device, po):
    sets = {k: R.wrapper_rows(k) for k in "ab"}
    want = {}
    for k, rows in sets.items():
        mn, mx = R.reference_bounds(rows)
        assert (mn < 0).all() and 17 in rows[:, 3]
        rig, pos, quat = R.wrapper_camera(rows)
        want[k] = U.visible_points_oracle(po, rows, np.repeat(rows[:, 3:4], 3, axis=1), rig, pos, quat, 0) + (rig, pos, quat)
        assert 0.2 < (want[k][0] >= 0).mean() < 0.9 and len(np.unique(want[k][0])) > 30
    dims = [tuple((R.reference_bounds(r)[1] - R.reference_bounds(r)[0]).tolist()) for r in sets.values()]
    assert dims[0] != dims[1] and 90 <= min(dims[0]) and max(dims[0]) <= 100
    dev_rows = {k: _to(cuda_device, r) for k, r in sets.items()}
    ws = {jumps: P.VolumeWorkspace(cuda_device) for jumps in (False, True)}
    for k in ("a", "b", "a"):          # the workspace grows for a, is reused larger than needed for b, and again for a
        vp_o, ins_o, rig, pos, quat = want[k]
        for jumps in (False, True):
            vp, ins = P.visible_point_map(dev_rows[k], rig, pos.copy(), quat, 0, use_jumps=jumps)
            assert np.array_equal(vp.cpu().numpy(), vp_o) and np.array_equal(ins.cpu().numpy(), ins_o), (k, jumps)
            vp, ins = P.visible_point_map(dev_rows[k], rig, pos.copy(), quat, 0, use_jumps=jumps, workspace=ws[jumps])
            assert np.array_equal(vp.cpu().numpy(), vp_o) and np.array_equal(ins.cpu().numpy(), ins_o), (k, jumps, "ws")
            assert int(ws[jumps].buf.count_nonzero()) == 0, (k, jumps)
    assert ws[True].buf.numel() == max((a + 1) * (b + 1) * (c + 2) for a, b, c in dims)
