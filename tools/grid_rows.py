"""What the hash-grid table gradient costs a single element: for every (case, path, dtype) of tests/test_grid_rows_gpu.py
the worst ratio to the tier-1 summation bound, and for float32 the tier-2 statistic (median, 99th percentile, maximum
of |got - sum64| / (2^-24 * abs64) over the elements with two contributions or more) of the GPU and of the C oracle and
their ratios -- the ratios are what the test bounds by 4.  One JSON line per (case, path, dtype); one process, each
case once (the deterministic path gives the same bits every time; the atomic paths reorder their sums from run to run).

    python tools/grid_rows.py > profiles/grid_rows.jsonl        (needs a GPU)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch


def main():
    import grid_rows as GR
    from test_grid_rows_gpu import DTYPES, RUNS
    dev = torch.device("cuda:0")
    for name, path, dt in RUNS:
        c, T = GR.case(name), DTYPES[dt]
        got = GR.gpu_backward(c, path, T, dev)
        sum64, abs64, n, bound = GR.path_bound(c, path, T)
        worst, bad = GR.tier1(got, sum64, abs64, n, bound)
        one = n == 1
        line = dict(case=name, path=path, dtype=dt, rows=c.rows, channels=c.C, longest_list=int(n.max()),
                    elements_n0=int((n == 0).sum()) * c.C, elements_n1=int(one.sum()) * c.C,
                    n0_exact_zero=not bool(got[n == 0].any()), n1_bit_exact=bool(np.array_equal(got[one], sum64[one].astype(T))),
                    tier1_worst=float("%.4g" % worst), tier1_beyond=bad)
        if T == np.float32:
            _, ost = c.oracle()
            st = GR.stats(GR.units(got, sum64, abs64, GR.U[T]), n)
            line.update(elements_n2=st["elements"], gpu={k: float("%.4g" % st[k]) for k in GR.STATS},
                        oracle={k: float("%.4g" % ost[k]) for k in GR.STATS},
                        ratio={k: round(v, 3) for k, v in GR.ratios(st, ost).items()}, within_4x=GR.within(st, ost))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
