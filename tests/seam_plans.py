"""The launch plan and the workspace formulas of the stage-seam operator (gcm_seam_*, gaussiancity_amd/csrc/gcm_seam.h's
seam_plan), transcribed into Python from the header's description, and PLAN_CASES: the large shapes of
tests/test_seam_plans_gpu.py with, per shape, the facts of the plan that the shape exists for.  tests/test_seam_host.py holds
the transcription to the library (both workspace queries agree over a sweep) and the facts to the transcription, as
tests/test_front_host.py does for tests/front_plans.py: if a constant of the plan changes, the host test names the case that
no longer reaches its branch."""
from gcm_plans import SUM_ROWS, _slices

T, KC = 64, 16
FOLD_TILES, MAX_GROUPS, MAX_SLICES = 64, 64, 64
MAX_CHANNELS = 512
CHUNK = 128           # kSeamChunk: inputs (forward) or outputs (dx) staged at a time; the widest column block


def _ceil(a, b):
    return -(-a // b)


def _round256(b):
    return _ceil(b, 256) * 256


def seam_plan(N, I, O):
    """tiles of 64 rows; G groups of gper consecutive tiles beyond 64 tiles (G = 1: one level); sw row slices of the weight
    gradient over wt tiles of 64 x 64, per rows each; the three pieces of the backward's workspace; and what
    gcm_seam_backward derives: the tiles of the last group, the slices without a row, the rows of the last slice that has
    any, and the chains of kFfnSumRows rows in the first slice."""
    tiles = _ceil(N, T)
    G = min(MAX_GROUPS, _ceil(tiles, FOLD_TILES)) if tiles > FOLD_TILES else 1
    gper = _ceil(tiles, G)
    wt = _ceil(O, T) * _ceil(I, T)
    cap = max(1, min(MAX_SLICES, 1024 // wt))
    sw = max(1, min(cap, _ceil(N, 64)))
    per = _ceil(_ceil(N, sw), KC) * KC
    part = _round256(max(tiles, 1) * 2 * O * 4)
    keep = _round256(2 * O * 4)
    wpart = _round256(sw * (O * I + O) * 4)
    p = {"tiles": tiles, "G": G, "gper": gper, "wt": wt, "cap": cap, "sw": sw, "per": per, "forward": part,
         "total": part + keep + wpart}
    p["last_group_tiles"] = tiles - (G - 1) * gper
    slices = _slices(N, sw)
    assert slices[0] == per
    p["empty_slices"], p["last_slice_rows"] = slices[1:]
    p["chains"] = _ceil(min(per, N), SUM_ROWS)
    return p


def facts(shape):
    """Every fact a PLAN_CASES entry may state, from the transcription."""
    N, I, O = shape
    p = seam_plan(N, I, O)
    return {"tiles": p["tiles"], "G": p["G"], "gper": p["gper"], "last_group_tiles": p["last_group_tiles"],
            "last_group_short": p["G"] >= 2 and 0 < p["last_group_tiles"] < p["gper"],
            "G_at_cap": p["G"] == MAX_GROUPS, "wt": p["wt"], "cap": p["cap"], "sw": p["sw"], "sw_at_cap": p["sw"] == p["cap"],
            "per": p["per"], "empty_slices": p["empty_slices"], "last_slice_rows": p["last_slice_rows"],
            "last_slice_short": 0 < p["last_slice_rows"] < p["per"], "chains": p["chains"],
            "chain_longer_than_sum_rows": p["chains"] >= 2,
            "input_chunks": _ceil(I, CHUNK), "output_chunks": _ceil(O, CHUNK), "part_column_blocks": _ceil(O, T)}


# (N, I, O) -> the facts the case exists for
PLAN_CASES = {
    # 65 tiles: two groups of 33 and 32; 64 slices of 80 rows, the last twelve without a row, slice 51 with 17 rows
    (4097, 4, 4): {"tiles": 65, "G": 2, "gper": 33, "last_group_tiles": 32, "last_group_short": True, "cap": 64, "sw": 64,
                   "sw_at_cap": True, "per": 80, "empty_slices": 12, "last_slice_rows": 17, "last_slice_short": True,
                   "chains": 3, "chain_longer_than_sum_rows": True},
    # 129 tiles: three groups of 43; widths between the templates
    (8193, 48, 36): {"tiles": 129, "G": 3, "gper": 43, "last_group_tiles": 43, "last_group_short": False, "sw": 64,
                     "sw_at_cap": True, "per": 144, "empty_slices": 7, "last_slice_short": True,
                     "chain_longer_than_sum_rows": True},
    # the measured workload shape: 256 tiles, four groups of exactly 64, every slice full
    (16384, 32, 64): {"tiles": 256, "G": 4, "gper": 64, "last_group_tiles": 64, "last_group_short": False, "sw": 64,
                      "sw_at_cap": True, "per": 256, "empty_slices": 0, "last_slice_rows": 256, "last_slice_short": False,
                      "chains": 8},
    # 4098 tiles: the groups at their cap, each longer than a one-level fold, the last with three tiles
    (262209, 4, 4): {"tiles": 4098, "G": 64, "G_at_cap": True, "gper": 65, "last_group_tiles": 3, "last_group_short": True,
                     "sw": 64, "sw_at_cap": True, "per": 4112, "chains": 129},
    # 32 weight tiles lower the cap to 32; four input chunks in the forward, two output chunks in dx, two column blocks
    (4097, 512, 256): {"G": 2, "last_group_short": True, "wt": 32, "cap": 32, "sw": 32, "sw_at_cap": True, "per": 144,
                       "empty_slices": 3, "last_slice_rows": 65, "last_slice_short": True, "input_chunks": 4,
                       "output_chunks": 2, "part_column_blocks": 4},
    # the same plan the other way: four column blocks, four chunks of dz, eight 64-column blocks in k_seam_bwd_part
    (4097, 256, 512): {"G": 2, "last_group_short": True, "wt": 32, "cap": 32, "sw": 32, "sw_at_cap": True, "per": 144,
                       "empty_slices": 3, "last_slice_rows": 65, "last_slice_short": True, "input_chunks": 2,
                       "output_chunks": 4, "part_column_blocks": 8},
    # 64 weight tiles: the cap is 16, without the grouped fold (33 tiles)
    (2049, 512, 512): {"tiles": 33, "G": 1, "wt": 64, "cap": 16, "sw": 16, "sw_at_cap": True, "per": 144, "empty_slices": 1,
                       "last_slice_rows": 33, "last_slice_short": True},
}
# the branch facts of the plan, each held by at least one case above (tests/test_seam_host.py)
BRANCH_FACTS = (("G >= 2 with a shorter last group", lambda f: f["G"] >= 2 and f["last_group_short"]),
                ("G at kSeamGroups with gper > 64", lambda f: f["G_at_cap"] and f["gper"] > FOLD_TILES),
                ("gper == 64 exactly in every group", lambda f: f["G"] >= 2 and f["gper"] == FOLD_TILES
                 and not f["last_group_short"]),
                ("sw at a cap of 64", lambda f: f["sw_at_cap"] and f["cap"] == MAX_SLICES),
                ("sw at a cap below 64", lambda f: f["sw_at_cap"] and f["cap"] < MAX_SLICES),
                ("the lowered cap without the grouped fold",
                 lambda f: f["sw_at_cap"] and f["cap"] < MAX_SLICES and f["G"] == 1),
                ("a slice without rows and a short last slice", lambda f: f["empty_slices"] >= 1 and f["last_slice_short"]),
                ("no slice without rows", lambda f: f["G"] >= 2 and f["empty_slices"] == 0),
                ("a weight-gradient chain longer than kFfnSumRows", lambda f: f["chain_longer_than_sum_rows"]),
                ("O > 128", lambda f: f["output_chunks"] >= 2),
                ("I > 128", lambda f: f["input_chunks"] >= 2))
# the shapes that also run without the product (width O), and the three whose statistics are checked at full weight
NO_PRODUCT_CASES = ((4097, 4, 4), (16384, 32, 64), (262209, 4, 4), (4097, 256, 512))
STATISTICS_CASES = ((4097, 4, 4), (16384, 32, 64), (262209, 4, 4))
