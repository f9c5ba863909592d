"""The device-resident volume path (gcv_points_bounds, gcv_rows_to_volume, gcv_rows_erase_volume, the occupancy bitmask),
the part that needs no GPU: every case of tests/rows_ref.py reaches the kernel path it is named for, the numpy reference
agrees with the oracle's points_to_volume on every case, the occupancy reference on a case written out by hand, the
argument checks that come back before any HIP call, and the two size queries."""
import ctypes as C
import os

import numpy as np
import pytest

import rows_ref as R
from gaussiancity_amd import _native_v as V
from oracle import points_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def po():
    PO.lib()
    return PO


def test_every_case_states_its_facts():
    assert set(R.CASE_FACTS) == set(R.CASES)
    for n in R.RAGGED_N:
        assert len(R.case("ragged_%d" % n)[0]) == n
    big = [name for name in R.CASES if R.case(name)[2:] == R.BIG]
    assert sorted(big) == ["many_words", "same_word"] and R.occupancy_bytes(*R.BIG) == 4 * 79
    for name in R.CASES:   # nothing larger than the two that have to be
        _, _, h, w, d = R.case(name)
        assert h * w * d <= R.BIG[0] * R.BIG[1] * R.BIG[2]


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_meets_its_facts(name):
    facts = R.case_facts(R.case(name))
    assert R.meets(facts, R.CASE_FACTS[name]) == [], facts


def test_meets_reports_a_miss():
    facts = {"a": 3, "b": (2, 0, 5), "c": 0.4}
    assert R.meets(facts, {"a": 3, "b": (2, 0, 5), "c": 0.4}) == []
    assert R.meets(facts, {"a": 4, "b": (1, 1, 1), "c": 0.51}) == [("a", 3, 4), ("b", (2, 0, 5), (1, 1, 1)), ("c", 0.4, 0.51)]


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_volume_is_the_oracle_on_localized_points(po, name):
    rows, offset, h, w, d = R.case(name)
    n = len(rows)
    want = po.points_to_volume(R.localize(rows, offset), np.arange(1, n + 1, dtype=np.int32),
                               np.repeat(rows[:, 3:4], 3, axis=1), h, w, d)
    vol, occ = R.reference(name)
    assert vol.dtype == np.int32 and vol.shape == (h, w, d) and np.array_equal(vol, want)
    assert occ.dtype == np.uint8 and occ.size == R.occupancy_bytes(h, w, d)
    if n == 0:
        assert not vol.any() and not occ.any()
    # explicit ids: in row order the two formulations are the same function
    assert np.array_equal(R.reference_points_volume(R.localize(rows, offset), np.arange(1, n + 1),
                                                    np.repeat(rows[:, 3:4], 3, axis=1), h, w, d), vol)


def test_reference_points_volume_highest_id_wins_in_any_row_order(po):
    rng = np.random.default_rng(8)
    h, w, d = 9, 12, 7
    n = 120
    pts = np.stack([rng.integers(-1, w + 1, n), rng.integers(-1, h + 1, n), rng.integers(-1, d + 1, n)], 1).astype(np.int16)
    sc = rng.integers(0, 6, (n, 3)).astype(np.int16)
    ids = (rng.permutation(n) * 7 + 3).astype(np.int32)
    got = R.reference_points_volume(pts, ids, sc, h, w, d)
    order = np.argsort(ids)
    assert np.array_equal(got, po.points_to_volume(pts[order], ids[order], sc[order], h, w, d))
    assert not np.array_equal(got, po.points_to_volume(pts, ids, sc, h, w, d))   # (the row order would differ)


def test_reference_occupancy_on_a_hand_written_case():
    """2 x 2 x 2 macro cells (h, w, d = 20, 17, 32); cell (kb, jb, lb) is bit (kb * 2 + jb) * 2 + lb."""
    vol = np.zeros((20, 17, 32), np.int32)
    assert R.reference_occupancy(vol).tolist() == [0, 0, 0, 0]
    vol[0, 0, 0] = 5         # cell (0, 0, 0) -> bit 0
    vol[15, 15, 31] = -1     # cell (0, 0, 1) -> bit 1 (any non-zero value counts)
    vol[16, 3, 16] = 9       # cell (1, 0, 1) -> bit 5
    vol[19, 16, 15] = 2      # cell (1, 1, 0) -> bit 6
    assert R.occupancy_cells(vol).tolist() == [True, True, False, False, False, True, True, False]
    assert R.reference_occupancy(vol).tolist() == [0b01100011, 0, 0, 0]
    vol[3, 16, 20] = 1       # cell (0, 1, 1) -> bit 3
    assert R.reference_occupancy(vol).tolist() == [0b01101011, 0, 0, 0]
    # 33 cells: the second word starts with cell 32, and whole words are returned
    long = np.zeros((1, 1, 33 * 16), np.int32)
    long[0, 0, 32 * 16] = 1
    long[0, 0, 9 * 16 + 15] = 1
    assert R.reference_occupancy(long).tolist() == [0, 2, 0, 0, 1, 0, 0, 0]


def test_reference_bounds_and_wrap():
    rows = np.array([[5, -7, 0, 1, 9], [-32768, 32767, 3, 1, 9], [4, 4, -2, 1, 9]], np.int16)
    mn, mx = R.reference_bounds(rows)
    assert mn.tolist() == [-32768, -7, -2] and mx.tolist() == [5, 32767, 3]
    assert R.localize(np.array([[30000, -30000, 7, 1, 0]], np.int16), (-10000, 10000, 8)).tolist() == [[-25536, 25536, -1]]


def _host_args():
    """Host memory in the roles of the device buffers: every call below fails a check before anything is read."""
    buf = (C.c_int32 * 4096)()
    return buf, C.addressof(buf)


def test_bounds_argument_errors_come_back_before_any_hip_call():
    lib = V.lib()
    buf, p = _host_args()
    mn, mx = (C.c_int32 * 3)(-7, -7, -7), (C.c_int32 * 3)(-7, -7, -7)

    def call(n=100, rows=p, stride=5, scratch=p, lo=mn, hi=mx):
        return lib.gcv_points_bounds(n, rows, stride, scratch, lo, hi, None)

    for kw in (dict(n=0), dict(n=-1), dict(rows=None), dict(scratch=None), dict(lo=None), dict(hi=None), dict(stride=2),
               dict(stride=1), dict(stride=0), dict(stride=-5)):
        assert call(**kw) == INVALID and b"gcv_points_bounds" in lib.gcv_last_error(), kw
    assert list(mn) == [-7, -7, -7] and list(mx) == [-7, -7, -7]
    with pytest.raises(RuntimeError, match="gcv_status -1"):
        V.check(call(n=0), "gcv_points_bounds")


def test_the_header_states_the_stride_the_code_accepts():
    header = " ".join(open(os.path.join(ROOT, "include", "gcv.h")).read().split())
    assert "`row_stride` elements (3 or 5)" not in header
    assert "`row_stride` >= 3 elements" in header


@pytest.mark.parametrize("entry", ["gcv_rows_to_volume", "gcv_rows_erase_volume"])
def test_rows_argument_errors_come_back_before_any_hip_call(entry):
    lib = V.lib()
    buf, p = _host_args()
    off = (C.c_int32 * 3)(0, 0, 0)

    def call(n=10, rows=p, offset=off, h=4, w=5, d=6, volume=p):
        if entry == "gcv_rows_to_volume":
            return lib.gcv_rows_to_volume(n, rows, offset, h, w, d, volume, None, 0, None)
        return lib.gcv_rows_erase_volume(n, rows, offset, h, w, d, volume, None)

    for kw in (dict(h=0), dict(w=0), dict(d=0), dict(h=-1), dict(w=-3), dict(d=-2 ** 31)):
        assert call(**kw) == INVALID and b"dimensions" in lib.gcv_last_error(), kw
    for kw in (dict(volume=None), dict(offset=None), dict(rows=None), dict(n=1, rows=None)):
        assert call(**kw) == INVALID and b"null" in lib.gcv_last_error(), kw
    assert call(n=-1) == INVALID
    if entry == "gcv_rows_to_volume":
        assert call(n=2 ** 31 - 1) == INVALID and b"2^31" in lib.gcv_last_error()
        assert call(n=2 ** 40) == INVALID
    else:
        assert call(n=0) == 0 and call(n=0, rows=None) == 0   # nothing to erase: nothing is enqueued
    assert not any(buf)


def test_size_queries_hold_their_formulas():
    lib = V.lib()
    assert lib.gcv_bounds_scratch_bytes() == 4 * 6 * 1024   # six ints for each of at most 1024 blocks
    for h in (-1, 0, 1, 15, 16, 17, 37, 300):
        for w in (0, 1, 16, 33, 300):
            for d in (-5, 0, 1, 31, 32, 100, 513):
                got = lib.gcv_occupancy_bytes(h, w, d)
                assert got == R.occupancy_bytes(h, w, d), (h, w, d)
                if min(h, w, d) <= 0:
                    assert got == 0
                else:
                    cells = -(-h // 16) * -(-w // 16) * -(-d // 16)
                    assert got % 4 == 0 and 8 * got >= cells > 8 * (got - 4)
    assert lib.gcv_occupancy_bytes(16, 16, 16 * 32) == 4 and lib.gcv_occupancy_bytes(16, 16, 16 * 32 + 1) == 8
    assert lib.gcv_occupancy_bytes(2048, 2048, 304) == 4 * ((128 * 128 * 19 + 31) // 32)
