"""The host-side launch plan of the Block-front backward, transcribed into Python from gaussiancity_amd/csrc/gcm_front.h
(front_plan), and PLAN_CASES: the large shapes of tests/test_front_gpu.py with, per shape, the facts of the plan that the
shape exists for.  tests/test_front_host.py holds the transcription to the library (the workspace totals agree over a
sweep) and the facts to the transcription, as tests/test_gcm_plans_host.py does for tests/gcm_plans.py."""
from gcm_plans import FOLD_TILES, KC, SUM_ROWS, T, _carve, _ceil, _slices  # noqa: F401

MAX_SLICES = 64       # kFfnMaxSlices: the leaves of the parameter fold's tree


def front_plan(N, C, O):
    """front_plan and what gcm_front_backward derives from it."""
    tiles = _ceil(N, T)
    groups = min(256, _ceil(tiles, FOLD_TILES)) if tiles > FOLD_TILES else 0
    wt = _ceil(max(O, C), T) * _ceil(C, T)                       # the grid of the larger weight gradient
    cap = max(1, min(MAX_SLICES, 1024 // wt))
    p = {"tiles": tiles, "groups": groups, "gper": _ceil(tiles, groups) if groups else 0, "cap": cap, "wt": wt,
         "sw": max(1, min(cap, _ceil(N, 64))), "record": O * C + C * C + O + C}
    p["last_group_tiles"] = tiles - (groups - 1) * p["gper"] if groups else 0
    p["per"], p["empty_slices"], p["last_slice_rows"] = _slices(N, p["sw"])
    p["chains"] = _ceil(min(p["per"], N), SUM_ROWS)             # chains of kFfnSumRows rows in the first slice
    p["launches"] = 4 + (1 if groups else 0)                    # rows, [group fold], LayerNorm fold, dw, parameter fold
    p["at"], p["total"] = _carve((("dt", N * C * 4), ("lnpart", tiles * 4 * C * 4), ("lngroup", groups * 4 * C * 4),
                                  ("wpart", p["sw"] * p["record"] * 4)))
    return p


def facts(shape):
    p = front_plan(*shape)
    return {"groups": p["groups"], "gper": p["gper"], "last_group_tiles": p["last_group_tiles"],
            "last_group_short": p["groups"] >= 2 and 0 < p["last_group_tiles"] < p["gper"],
            "sw": p["sw"], "sw_at_cap": p["sw"] == p["cap"], "per": p["per"], "empty_slices": p["empty_slices"],
            "last_slice_rows": p["last_slice_rows"], "last_slice_short": 0 < p["last_slice_rows"] < p["per"],
            "chain_longer_than_sum_rows": p["chains"] >= 2, "launches": p["launches"]}


# (N, C, O) -> the facts the case exists for
PLAN_CASES = {
    # 65 tiles: two groups of 33 and 32; 64 slices of 80 rows, the last twelve without a row, slice 51 with 17 rows
    (4097, 4, 12): {"groups": 2, "gper": 33, "last_group_tiles": 32, "last_group_short": True, "sw": 64, "sw_at_cap": True,
                    "per": 80, "empty_slices": 12, "last_slice_rows": 17, "last_slice_short": True,
                    "chain_longer_than_sum_rows": True, "launches": 5},
    # 129 tiles: three groups of 43
    (8193, 48, 40): {"groups": 3, "gper": 43, "last_group_tiles": 43, "sw": 64, "sw_at_cap": True, "per": 144,
                     "empty_slices": 7, "last_slice_short": True, "chain_longer_than_sum_rows": True, "launches": 5},
    # 12 weight tiles: the cap is still 64, and N reaches it
    (4097, 128, 384): {"groups": 2, "last_group_short": True, "sw": 64, "sw_at_cap": True, "per": 80, "empty_slices": 12,
                       "last_slice_short": True, "chain_longer_than_sum_rows": True, "launches": 5},
}
BRANCH_FACTS = (("groups >= 2 with a shorter last group", lambda f: f["groups"] >= 2 and f["last_group_short"]),
                ("sw at its cap", lambda f: f["sw_at_cap"]),
                ("a slice without rows and a short last slice", lambda f: f["empty_slices"] >= 1 and f["last_slice_short"]),
                ("a weight-gradient chain longer than kFfnSumRows", lambda f: f["chain_longer_than_sum_rows"]))
