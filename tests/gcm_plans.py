"""The two host-side launch plans of libgcm_hip.so, transcribed into Python from gaussiancity_amd/csrc/gcm_modlinear.hip
(plan_backward) and gcm_ffn.h (ffn_plan), and PLAN_CASES: the large shapes of tests/test_ffn_plans_gpu.py and
tests/test_modlinear_plans_gpu.py with, per shape, the facts of the plan that the shape exists for.

tests/test_gcm_plans_host.py holds the transcriptions to the library (the workspace totals agree over a sweep) and the
facts to the transcriptions, so a GPU case is tied to the branch it names without a GPU: if a constant of the plan
changes, the host test says which case no longer reaches its branch."""

T = 64                # rows of a workgroup tile, both libraries' products
KC = 16               # depth of a staged slice: a row slice is a multiple of it
SORT_ROWS = 256       # rows per block of the counting sort
SCAN_THREADS = 1024   # k_sort_scan: one workgroup, every thread a contiguous run of the counts
FOLD_TILES = 64       # kFfnFoldTiles: up to this many tiles fold in one level
SUM_ROWS = 32         # kFfnSumRows: rows of one chain of the feed-forward's weight gradients


def _ceil(a, b):
    return -(-a // b)


def _carve(sizes):
    """The offsets of the pieces, each rounded up to 256 bytes, and the total."""
    off, at = 0, {}
    for name, nbytes in sizes:
        at[name] = off
        off += _ceil(nbytes, 256) * 256
    return at, off


def _slices(N, sw):
    """Row slices of a weight gradient: rows per slice, the slices that have no row (p0 >= N) and the rows of the
    last slice that has any."""
    per = _ceil(_ceil(N, sw), KC) * KC
    empty = sum(1 for s in range(sw) if s * per >= N) if N else 0
    last = N - (sw - empty - 1) * per if N else 0
    return per, empty, last


def modlinear_plan(N, I, O, G):
    """plan_backward and what gcm_modlinear_backward derives from it."""
    tiles = _ceil(O, T) * _ceil(I, T)
    cap = max(1, min(64, 1024 // tiles))
    p = {"cap": cap, "sw": max(1, min(cap, _ceil(N, 128))), "sg": max(1, min(256, _ceil(N, 64 * G))),
         "nb": _ceil(N, SORT_ROWS)}
    p["per"], p["empty_slices"], p["last_slice_rows"] = _slices(N, p["sw"])
    p["counts"] = p["nb"] * G                                   # the (group, block) counts k_sort_scan scans
    p["run"] = _ceil(p["counts"], SCAN_THREADS)                 # ... and the counts one of its threads owns
    p["at"], p["total"] = _carve((("t", N * I * 4), ("wpart", p["sw"] * O * I * 4 if p["sw"] > 1 else 0),
                                  ("cnt", p["nb"] * G * 4), ("start", (G + 1) * 4), ("perm", N * 4),
                                  ("gpart", p["sg"] * G * (I + O) * 4)))
    return p


def ffn_plan(N, C, Hd):
    """ffn_plan and what gcm_ffn_backward derives from it."""
    tiles = _ceil(N, T)
    groups = min(256, _ceil(tiles, FOLD_TILES)) if tiles > FOLD_TILES else 0
    wt = _ceil(Hd, T) * _ceil(C, T)
    cap = max(1, min(64, 1024 // wt))
    p = {"tiles": tiles, "groups": groups, "gper": _ceil(tiles, groups) if groups else 0, "cap": cap,
         "sw": max(1, min(cap, _ceil(N, 64))), "record": 2 * C * Hd + Hd + C}
    p["last_group_tiles"] = tiles - (groups - 1) * p["gper"] if groups else 0
    p["per"], p["empty_slices"], p["last_slice_rows"] = _slices(N, p["sw"])
    p["chains"] = _ceil(min(p["per"], N), SUM_ROWS)             # chains of kFfnSumRows rows in the first slice
    p["at"], p["total"] = _carve((("da", N * Hd * 4), ("lnpart", tiles * 2 * C * 4), ("lngroup", groups * 2 * C * 4),
                                  ("wpart", p["sw"] * p["record"] * 4)))
    return p


def facts(kind, shape):
    """Every fact a PLAN_CASES entry may state, from the transcription."""
    if kind == "ffn":
        p = ffn_plan(*shape)
        return {"groups": p["groups"], "gper": p["gper"], "last_group_tiles": p["last_group_tiles"],
                "last_group_short": p["groups"] >= 2 and 0 < p["last_group_tiles"] < p["gper"],
                "sw": p["sw"], "sw_at_cap": p["sw"] == p["cap"], "per": p["per"], "empty_slices": p["empty_slices"],
                "last_slice_rows": p["last_slice_rows"], "last_slice_short": 0 < p["last_slice_rows"] < p["per"],
                "chain_longer_than_sum_rows": p["chains"] >= 2}
    p = modlinear_plan(*shape)
    return {"sw": p["sw"], "sw_at_cap": p["sw"] == p["cap"], "per": p["per"], "empty_slices": p["empty_slices"],
            "last_slice_rows": p["last_slice_rows"], "last_slice_short": 0 < p["last_slice_rows"] < p["per"],
            "sg": p["sg"], "nb": p["nb"], "counts": p["counts"], "run": p["run"],
            "count_loop_steps": _ceil(shape[3], SORT_ROWS)}


# (kind, shape) -> the facts the case exists for.  ffn shapes are (N, C, Hd), modlinear shapes (N, I, O, G).
PLAN_CASES = {
    # 65 tiles: two groups of 33 and 32; 64 slices of 80 rows, the last twelve without a row, slice 51 with 17 rows
    ("ffn", (4097, 4, 4)): {"groups": 2, "gper": 33, "last_group_tiles": 32, "last_group_short": True, "sw": 64,
                            "sw_at_cap": True, "per": 80, "empty_slices": 12, "last_slice_rows": 17,
                            "last_slice_short": True, "chain_longer_than_sum_rows": True},
    # 129 tiles: three groups of 43
    ("ffn", (8193, 48, 40)): {"groups": 3, "gper": 43, "last_group_tiles": 43, "sw": 64, "sw_at_cap": True, "per": 144,
                              "empty_slices": 7, "last_slice_short": True, "chain_longer_than_sum_rows": True},
    # 16 weight tiles: the cap is still 64, and N reaches it
    ("ffn", (4097, 128, 512)): {"groups": 2, "last_group_short": True, "sw": 64, "sw_at_cap": True, "per": 80,
                                "empty_slices": 12, "last_slice_short": True, "chain_longer_than_sum_rows": True},
    # 5 blocks x 300 groups = 1500 counts: a scan thread owns two, and group starts land inside a thread's run
    ("modlinear", (1025, 20, 36, 300)): {"nb": 5, "counts": 1500, "run": 2, "count_loop_steps": 2, "sw": 9, "per": 128,
                                         "last_slice_rows": 1, "sg": 1},
    # more groups than the scan has threads and than a count block has threads
    ("modlinear", (300, 4, 4, 1100)): {"nb": 2, "counts": 2200, "run": 3, "count_loop_steps": 5, "sg": 1},
    ("modlinear", (2049, 4, 4, 5)): {"nb": 9, "run": 1, "sw": 17, "per": 128, "empty_slices": 0, "last_slice_rows": 1,
                                     "last_slice_short": True, "sg": 7},
    # both slice counts at their caps; the longest chain of any plan here, 320 rows
    ("modlinear", (20000, 4, 4, 1)): {"sw": 64, "sw_at_cap": True, "per": 320, "empty_slices": 1, "last_slice_rows": 160,
                                      "last_slice_short": True, "sg": 256},
    # 64 weight tiles: the cap is 16
    ("modlinear", (2049, 512, 512, 5)): {"sw": 16, "sw_at_cap": True, "per": 144, "empty_slices": 1, "last_slice_rows": 33,
                                         "last_slice_short": True},
}
# the branch facts of the plans, each held by at least one case above (tests/test_gcm_plans_host.py)
BRANCH_FACTS = (("ffn", "groups >= 2 with a shorter last group", lambda f: f["groups"] >= 2 and f["last_group_short"]),
                ("ffn", "sw at its cap", lambda f: f["sw_at_cap"]),
                ("ffn", "a slice without rows and a short last slice", lambda f: f["empty_slices"] >= 1 and f["last_slice_short"]),
                ("ffn", "a weight-gradient chain longer than kFfnSumRows", lambda f: f["chain_longer_than_sum_rows"]),
                ("modlinear", "sw at its cap", lambda f: f["sw_at_cap"]),
                ("modlinear", "a slice without rows and a short last slice",
                 lambda f: f["empty_slices"] >= 1 and f["last_slice_short"]),
                ("modlinear", "scan run >= 2", lambda f: f["run"] >= 2),
                ("modlinear", "more groups than a count block has threads", lambda f: f["count_loop_steps"] >= 2),
                ("modlinear", "sg == 256", lambda f: f["sg"] == 256))


def cases(kind):
    return [shape for (k, shape) in PLAN_CASES if k == kind]
