"""The device-resident volume path of libgcv_hip.so (gcv_points_bounds, gcv_rows_to_volume, gcv_rows_erase_volume and the
occupancy bitmask) in plain numpy, and CASES: small row sets with, per case, the facts it exists for.

tests/test_rows_volume_host.py holds reference_volume to the oracle's points_to_volume on every case and every case to
CASE_FACTS, so a GPU case of tests/test_rows_volume_gpu.py is tied to the kernel path it names without a GPU: if a
generator or a seed changes, the host test says which case no longer reaches its path.  Everything is integer work."""
import functools

import numpy as np

MC = 16     # side of a macro cell (MC_SHIFT = 4 in gaussiancity_amd/csrc/gcv_points.hip)
WAVE = 64   # rows 64 k .. 64 k + 63 are the lanes of one wave (256-thread blocks, one row per thread)


def localize(rows, offset):
    """Columns 0..2 minus the offset, wrapped to int16 as the reference's tensor ops wrap."""
    return (rows[:, :3].astype(np.int32) - np.asarray(offset, np.int32)).astype(np.int16)


def _cubes(loc, scales3, h, w, d):
    """Per row: does it write anything, and the clipped cube [lo, hi) in (x, y, z)."""
    loc, sc = loc.astype(np.int64).reshape(-1, 3), scales3.astype(np.int64).reshape(-1, 3)
    dims = np.array([w, h, d], np.int64)
    hi = np.minimum(loc + sc, dims)
    valid = ((loc >= 0) & (loc < dims)).all(1) & (hi > loc).all(1)
    return valid, loc, hi


def _write(order, ids, valid, lo, hi, h, w, d):
    vol = np.zeros((h, w, d), np.int32)
    for i in order:
        if valid[i]:
            vol[lo[i, 1]:hi[i, 1], lo[i, 0]:hi[i, 0], lo[i, 2]:hi[i, 2]] = ids[i]
    return vol


def reference_volume(rows, offset, h, w, d):
    """gcv_rows_to_volume: id = row index + 1, cube side = column 3, written in row order (the highest row wins)."""
    n = len(rows)
    valid, lo, hi = _cubes(localize(rows, offset), np.repeat(rows[:, 3:4], 3, axis=1), h, w, d)
    return _write(range(n), np.arange(1, n + 1, dtype=np.int32), valid, lo, hi, h, w, d)


def reference_points_volume(points, ids, scales, h, w, d):
    """gcv_points_to_volume with explicit ids and per-axis scales: written in ascending id, so the highest id wins
    whatever the row order (ids are distinct)."""
    ids = np.asarray(ids, np.int32).reshape(-1)
    valid, lo, hi = _cubes(points, scales, h, w, d)
    return _write(np.argsort(ids, kind="stable"), ids, valid, lo, hi, h, w, d)


def occupancy_cells(volume):
    """bool [hb * wb * db]: which 16^3 macro cells hold a non-zero voxel, in the bitmask's order."""
    h, w, d = volume.shape
    hb, wb, db = (h + MC - 1) // MC, (w + MC - 1) // MC, (d + MC - 1) // MC
    pad = np.zeros((hb * MC, wb * MC, db * MC), bool)
    pad[:h, :w, :d] = volume != 0
    return pad.reshape(hb, MC, wb, MC, db, MC).any(axis=(1, 3, 5)).reshape(-1)


def occupancy_bytes(h, w, d):
    """gcv_occupancy_bytes: one bit per macro cell, whole 32-bit words; 0 for a non-positive dimension."""
    if h <= 0 or w <= 0 or d <= 0:
        return 0
    cells = ((h + MC - 1) // MC) * ((w + MC - 1) // MC) * ((d + MC - 1) // MC)
    return 4 * ((cells + 31) // 32)


def reference_occupancy(volume):
    """uint8 [gcv_occupancy_bytes]: bit i (little-endian within each byte) = macro cell i holds a non-zero voxel."""
    cells = occupancy_cells(volume)
    bits = np.zeros(8 * occupancy_bytes(*volume.shape), np.uint8)
    bits[:cells.size] = cells
    return np.packbits(bits, bitorder="little")


def reference_bounds(rows):
    """gcv_points_bounds: (min[3], max[3]) of columns 0..2."""
    p = rows[:, :3].astype(np.int32)
    return p.min(0), p.max(0)


# ---- the cases --------------------------------------------------------------------------------------------------
BIG = (300, 300, 100)   # h, w, d: 19 x 19 x 7 = 2 527 macro cells = 79 bitmask words, 36 MB


def _rows(x, y, z, s, seed):
    n = len(x)
    ins = np.random.default_rng(seed).integers(1, 300, n)
    a = np.stack([np.asarray(v, np.int64) for v in (x, y, z, s, ins)], 1).reshape(n, 5)
    assert n == 0 or (a.min() >= -32768 and a.max() <= 32767)   # a case wraps where it says so, nowhere else
    return a.astype(np.int16)


def _stored(local, offset):
    """The int16 value that the subtraction of `offset` turns into `local` (through a wrap where it has to)."""
    return (np.asarray(local, np.int64) + offset + 32768) % 65536 - 32768


def _many_words():
    rng = np.random.default_rng(101)
    h, w, d = BIG
    n = 4096 + 37
    return _rows(rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, d, n), rng.integers(1, 4, n), 1), (0, 0, 0), h, w, d


def _same_word():
    """Every wave inside one macro cell of its own (the last wave is partial); cubes of side 1 and 2, so a few of them
    reach into the neighbouring cell."""
    rng = np.random.default_rng(102)
    h, w, d = BIG
    waves, last = 40, 29
    cell = np.stack([rng.integers(0, w // MC, waves + 1), rng.integers(0, h // MC, waves + 1), rng.integers(0, d // MC, waves + 1)], 1)
    cell = np.repeat(cell, WAVE, axis=0)[: waves * WAVE + last]
    p = cell * MC + rng.integers(0, MC, cell.shape)
    return _rows(p[:, 0], p[:, 1], p[:, 2], rng.integers(1, 3, len(p)), 2), (0, 0, 0), h, w, d


def _invalid_lanes():
    """About a third of the lanes of every wave write nothing: outside the volume or without a positive scale."""
    rng = np.random.default_rng(103)
    h, w, d = 100, 90, 70
    n = 1500
    x, y, z = rng.integers(-12, w + 12, n), rng.integers(-12, h + 12, n), rng.integers(-6, d + 6, n)
    s = rng.integers(-1, 6, n)
    return _rows(x + 7, y - 5, z + 3, s, 3), (7, -5, 3), h, w, d


def _big_cubes():
    """Sides 1, 15, 16, 17, 33 and 40 at 0, 15 and 16 within a macro cell, every combination of the three axes."""
    rng = np.random.default_rng(104)
    h, w, d = 96, 112, 80
    x, y, z, s = [], [], [], []
    for side in (1, 15, 16, 17, 33, 40):
        for ax in (0, 15, 16):
            for ay in (0, 15, 16):
                for az in (0, 15, 16):
                    x.append(MC * int(rng.integers(0, 4)) + ax)
                    y.append(MC * int(rng.integers(0, 3)) + ay)
                    z.append(MC * int(rng.integers(0, 2)) + az)
                    s.append(side)
    order = rng.permutation(len(s))
    x, y, z, s = (np.array(v)[order] for v in (x, y, z, s))
    return _rows(x - 40, y - 3, z + 9, s, 4), (-40, -3, 9), h, w, d


def _faces():
    """No dimension is a multiple of 16; cubes end in, and are cut by, the last partial macro cell of every axis."""
    rng = np.random.default_rng(105)
    h, w, d = 37, 50, 21
    hand = [(0, 0, 0, 1), (0, 0, 0, 5), (w - 1, 0, 0, 1), (0, h - 1, 0, 1), (0, 0, d - 1, 1), (w - 1, h - 1, d - 1, 1),
            (w - 1, h - 1, d - 1, 9), (w - 1, 3, 4, 3), (5, h - 1, 2, 4), (7, 9, d - 1, 2),   # start at dim - 1, cut at once
            (48, 10, 3, 2), (48, 10, 3, 3), (47, 20, 5, 3), (47, 20, 5, 4),                   # w: last cell is 48..49
            (10, 33, 3, 4), (10, 33, 3, 5), (20, 31, 5, 6), (20, 31, 5, 7),                   # h: last cell is 32..36
            (10, 10, 17, 4), (10, 10, 17, 5), (20, 5, 15, 6), (20, 5, 15, 7),                 # d: last cell is 16..20
            (40, 30, 12, 17), (0, 0, 0, 40), (33, 0, 0, 17), (0, 21, 0, 17), (0, 0, 5, 17)]
    m = 150
    x = np.concatenate([[v[0] for v in hand], rng.integers(0, w, m)])
    y = np.concatenate([[v[1] for v in hand], rng.integers(0, h, m)])
    z = np.concatenate([[v[2] for v in hand], rng.integers(0, d, m)])
    s = np.concatenate([[v[3] for v in hand], rng.integers(1, 7, m)])
    order = rng.permutation(len(s))
    return _rows(x[order], y[order], z[order], s[order], 5), (0, 0, 0), h, w, d


def _dropped():
    """Rows that write nothing, one kind each and then at random, between rows that do.  Offsets (10000, -10000, 0):
    x = -30000 wraps INTO the volume (-40000 -> 25536 < w), y = 30000 wraps OUT of it (40000 -> -25536).  With
    w + 10000 > 32767 a row beyond the upper x face is itself one that wrapped."""
    rng = np.random.default_rng(106)
    h, w, d = 3, 25600, 4
    ox, oy, oz = 10000, -10000, 0
    hand = [(-1, 0, 0, 1), (w, 0, 0, 1), (0, -1, 0, 1), (0, h, 0, 1), (0, 0, -1, 1), (0, 0, d, 1),   # localized coordinates
            (5, 1, 1, 0), (6, 1, 1, -1), (7, 1, 1, -32768), (w + 7000, 1, 1, 2), (-9000, 2, 2, 2)]
    m = 200
    lx = np.concatenate([[v[0] for v in hand], rng.integers(-50, w + 50, m)])
    ly = np.concatenate([[v[1] for v in hand], rng.integers(-1, h + 1, m)])
    lz = np.concatenate([[v[2] for v in hand], rng.integers(-1, d + 1, m)])
    s = np.concatenate([[v[3] for v in hand], rng.integers(-1, 4, m)])
    x, y, z = _stored(lx, ox), _stored(ly, oy), _stored(lz, oz)
    # the wrapping rows, as stored values: (x, y, z, scale)
    wrap = [(-30000, oy + 1, 1, 2), (-30000 + 63, oy, 0, 3), (-30000 - 2000, oy + 2, 3, 1),   # into the volume
            (ox + 9, 30000, 1, 2), (ox + 10, 22768, 2, 2), (ox + 11, 32767, 0, 1),            # out of it, through y
            (-32768, oy, 0, 1)]                                                               # -42768 -> 22768: in
    x = np.concatenate([x, [v[0] for v in wrap]])
    y = np.concatenate([y, [v[1] for v in wrap]])
    z = np.concatenate([z, [v[2] for v in wrap]])
    s = np.concatenate([s, [v[3] for v in wrap]])
    order = rng.permutation(len(s))
    return _rows(x[order], y[order], z[order], s[order], 6), (ox, oy, oz), h, w, d


def _overlaps():
    rng = np.random.default_rng(107)
    h, w, d = 24, 20, 18
    n = 700
    return _rows(rng.integers(-900, w - 900, n), rng.integers(50, h + 50, n), rng.integers(0, d, n), rng.integers(2, 9, n), 7), (-900, 50, 0), h, w, d


def _ragged(n):
    def make():
        rng = np.random.default_rng(200 + n)
        h, w, d = 21, 35, 19
        return _rows(rng.integers(-1, w + 1, n) - 3, rng.integers(-1, h + 1, n) + 4, rng.integers(-1, d + 1, n), rng.integers(0, 5, n), 8), (-3, 4, 0), h, w, d
    return make


RAGGED_N = (0, 1, 63, 64, 65, 255, 257)
CASES = {"many_words": _many_words, "same_word": _same_word, "invalid_lanes": _invalid_lanes, "big_cubes": _big_cubes,
         "faces": _faces, "dropped": _dropped, "overlaps": _overlaps}
CASES.update({"ragged_%d" % n: _ragged(n) for n in RAGGED_N})


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(name):
    """(rows int16 [n, 5], offset, h, w, d) of a CASES entry; made once, read-only."""
    rows, offset, h, w, d = CASES[name]()
    assert rows.dtype == np.int16 and rows.shape[1] == 5
    return _frozen(np.ascontiguousarray(rows)), tuple(int(v) for v in offset), int(h), int(w), int(d)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(volume, occupancy bytes) of a case from the reference; made once, read-only."""
    vol = reference_volume(*case(name))
    return _frozen(vol), _frozen(reference_occupancy(vol))


# ---- what each case exists for ----------------------------------------------------------------------------------
def case_facts(c):
    """The facts a CASE_FACTS entry may state, from the reference alone."""
    rows, offset, h, w, d = c
    n = len(rows)
    dims = np.array([w, h, d], np.int64)
    exact = rows[:, :3].astype(np.int64) - np.asarray(offset, np.int64)
    loc = localize(rows, offset).astype(np.int64)
    s = rows[:, 3].astype(np.int64)
    valid, lo, hi = _cubes(loc, np.repeat(rows[:, 3:4], 3, axis=1), h, w, d)
    wrapped = (exact != loc).any(1)
    inside = ((loc >= 0) & (loc < dims)).all(1)
    f = {"rows": n, "valid_rows": int(valid.sum())}
    # the word of the bitmask a lane hands to the wave-level merge (the macro cell of the cube's first voxel)
    wb, db = (w + MC - 1) // MC, (d + MC - 1) // MC
    word = (((lo[:, 1] // MC) * wb + lo[:, 0] // MC) * db + lo[:, 2] // MC) // 32
    per_wave, one_word, full_one_word, mixed = [0], 0, 0, 0
    for k in range(0, n, WAVE):
        v = valid[k:k + WAVE]
        words = np.unique(word[k:k + WAVE][v])
        per_wave.append(len(words))
        one_word += int(len(words) == 1)
        full_one_word += int(len(words) == 1 and int(v.sum()) == WAVE)
        mixed += int(v.any() and not v.all())
    f["max_words_in_a_wave"] = max(per_wave)
    f["one_word_waves"], f["full_one_word_waves"], f["mixed_waves"] = one_word, full_one_word, mixed
    span = (hi[valid] - 1) // MC - lo[valid] // MC + 1 if valid.any() else np.zeros((1, 3), np.int64)
    f["max_span"] = tuple(int(v) for v in span.max(0))
    cut = valid[:, None] & (loc + s[:, None] > dims)
    f["clipped"] = tuple(int(v) for v in cut.sum(0))   # by the upper x, y and z face
    in_partial = (dims % MC != 0) & (lo // MC == (dims - 1) // MC)   # starts in a last macro cell that is cut short
    f["clipped_from_the_partial_cell"] = tuple(int(v) for v in (cut & in_partial).sum(0))
    f["start_at_zero"] = tuple(int(v) for v in (valid[:, None] & (loc == 0)).sum(0))
    f["start_at_last"] = tuple(int(v) for v in (valid[:, None] & (loc == dims - 1)).sum(0))
    f["dropped_low"] = tuple(int(v) for v in (loc < 0).sum(0))        # x, y, z, as the kernel sees them
    f["dropped_high"] = tuple(int(v) for v in (loc >= dims).sum(0))
    f["dropped_scale"] = int((inside & (s <= 0)).sum())
    f["wrapped_out"] = int((wrapped & ~inside).sum())
    f["wrapped_in"] = int((wrapped & valid).sum())
    writers = np.zeros((h, w, d), np.int32)
    for i in np.nonzero(valid)[0]:
        writers[lo[i, 1]:hi[i, 1], lo[i, 0]:hi[i, 0], lo[i, 2]:hi[i, 2]] += 1
    written = int((writers > 0).sum())
    f["written_voxels"] = written
    f["multi_writer_share"] = float((writers > 1).sum()) / written if written else 0.0
    occupied = occupancy_cells(writers).reshape((h + MC - 1) // MC, wb, db)
    # macro cells by how the kernel reaches them: as a cube's first cell (the wave merge), as one of the first two of
    # a span on every axis, or only as a third or later one; and the empty cell right behind a cube that ends flush
    # with a macro-cell face, which a loop running one cell too far would set
    first, two = np.zeros_like(occupied), np.zeros_like(occupied)
    flush = 0
    for i in np.nonzero(valid)[0]:
        c0, c1 = lo[i] // MC, (hi[i] - 1) // MC
        first[c0[1], c0[0], c0[2]] = True
        c2 = np.minimum(c1, c0 + 1)
        two[c0[1]:c2[1] + 1, c0[0]:c2[0] + 1, c0[2]:c2[2] + 1] = True
        if (c1 > c0).any():
            for a in range(3):
                nxt = c0.copy()
                nxt[a] = c1[a] + 1
                if hi[i, a] % MC == 0 and hi[i, a] < dims[a] and not occupied[nxt[1], nxt[0], nxt[2]]:
                    flush += 1
    f["cells_only_by_straddle"] = int((occupied & ~first).sum())
    f["cells_only_beyond_the_second"] = int((occupied & ~two).sum())
    f["flush_cubes_before_an_empty_cell"] = flush
    return f


# The least each case must reach (tuples element by element); behind each, the figure when this was written.
CASE_FACTS = {
    "many_words": {"max_words_in_a_wave": 32,                    # 49 of the volume's 79: the merge loop runs 49 times
                   "cells_only_by_straddle": 1,                  # 127
                   "flush_cubes_before_an_empty_cell": 1},       # 15
    "same_word": {"full_one_word_waves": 1,                      # 40
                  "one_word_waves": 2,                           # 41: the partial last wave too
                  "flush_cubes_before_an_empty_cell": 1},        # 3
    "invalid_lanes": {"mixed_waves": 20,                         # 24, every wave
                      "max_words_in_a_wave": 3,                  # 7, every word of the volume
                      "dropped_scale": 1},                       # 219
    "big_cubes": {"max_span": (3, 3, 3),                         # (4, 4, 4)
                  "cells_only_beyond_the_second": 1,             # 89
                  "max_words_in_a_wave": 3},                     # 4
    "faces": {"clipped_from_the_partial_cell": (1, 1, 1),        # (7, 15, 17)
              "start_at_zero": (1, 1, 1),                        # (11, 12, 14)
              "start_at_last": (1, 1, 1),                        # (6, 11, 11)
              "max_span": (3, 3, 2)},                            # (3, 3, 2): d has two cells
    "dropped": {"dropped_low": (1, 1, 1),                        # (2, 43, 37)
                "dropped_high": (1, 1, 1),                       # (2, 47, 34); x only through a wrap, see _dropped
                "dropped_scale": 1,                              # 30
                "wrapped_out": 1,                                # 17
                "wrapped_in": 1,                                 # 12
                "valid_rows": 1},                                # 56
    "overlaps": {"multi_writer_share": 0.51,                     # 0.939
                 "valid_rows": 700},                             # 700
}
CASE_FACTS.update({"ragged_%d" % n: {"rows": n} for n in RAGGED_N})


def meets(facts, minimum):
    """[(fact, got, want)] for every fact of `minimum` that `facts` misses."""
    miss = []
    for k, want in minimum.items():
        got = facts[k]
        ok = all(g >= m for g, m in zip(got, want)) if isinstance(want, tuple) else got >= want
        if not ok:
            miss.append((k, got, want))
    return miss


# ---- row sets for the wrapper (points.visible_point_map works out the volume from the rows' own bounds) -----------
def wrapper_rows(which):
    """int16 [n, 5] rows as the extruder writes them, but adversarial: negative coordinates (so negative offsets),
    sides 1..5 and 17, cubes piled on each other.  'a': about 100^3 voxels; 'b': fewer rows, another extent."""
    rng = np.random.default_rng({"a": 301, "b": 302}[which])
    n, lo, hi = {"a": (420, (-61, -48, -23), (38, 51, 70)), "b": (150, (-30, -81, -9), (29, -10, 41))}[which]
    p = np.stack([rng.integers(lo[a], hi[a] + 1, n) for a in range(3)], 1)
    p[: n // 3, 2] = lo[2] + rng.integers(0, 3, n // 3)            # a floor of cubes, most of them overlapping
    p[0], p[1] = lo, hi                                            # the bounds are met, by one row each
    s = rng.choice(np.array([1, 2, 3, 5, 17]), n, p=[0.2, 0.2, 0.2, 0.2, 0.2])
    return _frozen(_rows(p[:, 0], p[:, 1], p[:, 2], s, 9))


def wrapper_camera(rows, W=96, H=56):
    """(cam_rig, cam_pos, cam_quat): above and beside the rows' box, looking at its centre."""
    from gaussiancity_amd import synth
    mn, mx = reference_bounds(rows)
    centre = (mn + mx) / 2.0
    pos = centre + np.array([1.1, -0.9, 1.3]) * (mx - mn)
    f = 0.8 * W
    rig = {"intrinsics": [f, 0.0, W / 2.0, 0.0, f, H / 2.0, 0.0, 0.0, 1.0], "sensor_size": [W, H]}
    return rig, pos.astype(np.float64), synth.quat_from_look_at(pos, centre)
