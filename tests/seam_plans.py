"""The launch plan and the workspace formulas of the stage-seam operator (gcm_seam_*, gaussiancity_amd/csrc/gcm_seam.h's
seam_plan), transcribed into Python from the header's description: tests/test_seam_host.py holds the library to them."""
T, KC = 64, 16
FOLD_TILES, MAX_GROUPS, MAX_SLICES = 64, 64, 64
MAX_CHANNELS = 512


def _ceil(a, b):
    return -(-a // b)


def _round256(b):
    return _ceil(b, 256) * 256


def seam_plan(N, I, O):
    """tiles of 64 rows; G groups of gper consecutive tiles beyond 64 tiles (G = 1: one level); sw row slices of the weight
    gradient over wt tiles of 64 x 64, per rows each; the three pieces of the backward's workspace."""
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
    return {"tiles": tiles, "G": G, "gper": gper, "wt": wt, "sw": sw, "per": per, "forward": part,
            "total": part + keep + wpart}
