"""The host-side plan of the split feed-forward entry points (gcm_ffn_split_*), transcribed into Python from
gaussiancity_amd/csrc/gcm_ffn.h (ffn_plan with records), in the style of tests/gcm_plans.py.  The mode limit is a tuning constant
of the library: the transcription takes it from the plan query (plan[6]) and never states it.

tests/test_ffn_split_host.py holds the transcription to the library over a grid of shapes."""
from gcm_plans import FOLD_TILES, T, _carve, _ceil

FH = 64               # hidden features per chunk


def split_plan(N, C, Hd, limit):
    """ffn_plan with records: the mode, the records and both workspaces."""
    tiles, chunks = _ceil(N, T), _ceil(Hd, FH)
    split = tiles * chunks <= limit
    records = chunks if split else 1
    groups = min(256, _ceil(tiles, FOLD_TILES)) if tiles > FOLD_TILES else 0
    wt = _ceil(Hd, T) * _ceil(C, T)
    sw = max(1, min(max(1, min(64, 1024 // wt)), _ceil(N, 64)))
    rec = records * N * C * 4
    p = {"mode": 1 if split else 0, "tiles": tiles, "chunks": chunks, "records": records, "sw": sw, "groups": groups,
         "limit": limit, "forward": max(256, _ceil(rec, 256) * 256)}
    p["at"], p["backward"] = _carve((("da", N * Hd * 4), ("part", rec), ("lnpart", tiles * 2 * C * 4),
                                     ("lngroup", groups * 2 * C * 4), ("wpart", sw * (2 * C * Hd + Hd + C) * 4)))
    return p


def as_query(p):
    """The eight numbers gcm_ffn_split_plan writes."""
    return [p["mode"], p["tiles"], p["chunks"], p["records"], p["sw"], p["groups"], p["limit"], 0]


def first_rows_mode_n(Hd, limit):
    """The smallest N the plan puts in rows mode at this hidden width."""
    return T * (limit // _ceil(Hd, FH)) + 1
