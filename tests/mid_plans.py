"""The host-side launch plan of the Block-middle backward, transcribed into Python from gaussiancity_amd/csrc/gcm_mid.h
(mid_plan) and gcm_mid_backward.  tests/test_mid_host.py holds the transcription to the library: the workspace totals agree
over a sweep of (N, C), as tests/test_front_host.py does for tests/front_plans.py."""
from gcm_plans import KC, SUM_ROWS, T, _carve, _ceil, _slices  # noqa: F401

MAX_SLICES = 64       # kFfnMaxSlices: the leaves of the parameter fold's tree


def mid_plan(N, C, da=True, params=True):
    """mid_plan and what gcm_mid_backward derives from it; da, params: the outputs asked for."""
    wt = _ceil(C, T) ** 2                                       # 64 x 64 tiles of dWp
    cap = max(1, min(MAX_SLICES, 1024 // wt))
    p = {"tiles": _ceil(N, T), "wt": wt, "cap": cap, "sw": max(1, min(cap, _ceil(N, 64))), "record": C * C + C}
    p["per"], p["empty_slices"], p["last_slice_rows"] = _slices(N, p["sw"])
    p["chains"] = _ceil(min(p["per"], N), SUM_ROWS)             # chains of kFfnSumRows rows in the first slice
    p["launches"] = (1 if da else 0) + (2 if params else 0)     # rows; dw, parameter fold
    p["at"], p["total"] = _carve((("wpart", p["sw"] * p["record"] * 4),))
    return p
