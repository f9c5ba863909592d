"""The launch plans of libgcm_hip.so without a GPU (not gpu).  tests/gcm_plans.py transcribes plan_backward
(gcm_modlinear.hip) and ffn_plan (gcm_ffn.h); here each transcription's carve is held to the library's own workspace query
over a sweep of shapes, and every entry of PLAN_CASES -- the large shapes the two *_plans_gpu.py files run -- is held to
the facts it states: which fold level, which slice count at its cap, which slices without rows, which scan run.  A case
that no longer reaches the branch it names fails here, on the CPU."""
import pytest

import gcm_plans as P
from gaussiancity_amd import _native_m as M

NS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 65536)
FFN_WIDTHS = ((4, 4), (32, 128), (48, 40), (128, 512), (36, 144), (68, 64), (100, 400), (128, 8), (4, 512), (64, 256))
MOD_WIDTHS = ((4, 4, 1), (4, 4, 5), (20, 36, 5), (20, 36, 300), (4, 4, 1100), (64, 64, 5), (512, 512, 5), (512, 512, 16))


def test_the_ffn_transcription_carves_what_the_library_asks_for():
    lib = M.lib()
    shapes = [(N, C, Hd) for (C, Hd) in FFN_WIDTHS for N in NS + (130, 8193)] + P.cases("ffn")
    for shape in shapes:
        p = P.ffn_plan(*shape)
        assert lib.gcm_ffn_backward_workspace_bytes(*shape) == p["total"], (shape, p)
        assert all(off % 256 == 0 for off in p["at"].values()) and p["total"] % 256 == 0
        assert (p["groups"] == 0) == (shape[0] <= 4096), shape          # the second fold level starts past 64 tiles


def test_the_modlinear_transcription_carves_what_the_library_asks_for():
    lib = M.lib()
    shapes = [(N, I, O, G) for (I, O, G) in MOD_WIDTHS for N in NS + (333, 1025, 2049, 20000)] + P.cases("modlinear")
    for shape in shapes:
        p = P.modlinear_plan(*shape)
        assert lib.gcm_modlinear_backward_workspace_bytes(*shape) == p["total"], (shape, p)
        assert all(off % 256 == 0 for off in p["at"].values()) and p["total"] % 256 == 0


def test_the_slices_cover_every_row_once_and_the_groups_every_tile_once():
    for kind, shape in P.PLAN_CASES:
        p = P.ffn_plan(*shape) if kind == "ffn" else P.modlinear_plan(*shape)
        N, rows = shape[0], 0
        for s in range(p["sw"]):
            p0 = s * p["per"]
            rows += max(min(p0 + p["per"], N) - p0, 0)
        assert rows == N and p["per"] % P.KC == 0, (kind, shape, p)
        if kind == "ffn" and p["groups"]:
            tiles = sum(max(min((q + 1) * p["gper"], p["tiles"]) - q * p["gper"], 0) for q in range(p["groups"]))
            assert tiles == p["tiles"] and (p["groups"] - 1) * p["gper"] < p["tiles"], (shape, p)


@pytest.mark.parametrize("kind,shape", sorted(P.PLAN_CASES))
def test_every_plan_case_reaches_the_branch_it_names(kind, shape):
    stated, derived = P.PLAN_CASES[(kind, shape)], P.facts(kind, shape)
    assert stated and set(stated) <= set(derived)
    wrong = {k: (v, derived[k]) for k, v in stated.items() if derived[k] != v}
    assert not wrong, (kind, shape, wrong)


@pytest.mark.parametrize("kind,name", [(k, n) for k, n, _ in P.BRANCH_FACTS])
def test_every_branch_fact_is_held_by_a_case(kind, name):
    holds = [f for k, n, f in P.BRANCH_FACTS if (k, n) == (kind, name)][0]
    holding = [shape for shape in P.cases(kind) if holds(P.facts(kind, shape))]
    print(kind, name, holding)
    assert holding, (kind, name)


def test_the_small_shapes_of_the_older_tests_reach_none_of_these_branches():
    """What the suite ran before: one fold level, no slice without rows, one count per scan thread."""
    for C, Hd in ((4, 4), (32, 128), (48, 40), (128, 512)):
        f = P.facts("ffn", (257, C, Hd))
        assert f["groups"] == 0 and f["empty_slices"] == 0 and not f["sw_at_cap"], (C, Hd, f)
    for I, O in ((4, 4), (20, 36), (64, 64)):
        f = P.facts("modlinear", (333, I, O, 5))
        assert f["run"] == 1 and f["count_loop_steps"] == 1 and f["empty_slices"] == 0 and f["sg"] < 256 and not f["sw_at_cap"]
