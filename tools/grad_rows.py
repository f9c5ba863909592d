"""What the backward costs a single Gaussian: for every scene and kernel variant of tests/grad_rows.py, the per-row
relative error (median, 99th percentile, maximum over the Gaussians with a non-zero reference) of the binary32 oracle and
of the GPU against the state-consistent binary64 reference (oracle.Frame64.from_frame), and their ratios -- the ratios
are what tests/test_gpu_grad_rows.py bounds by 4.  One JSON line per (scene, variant, tensor).

    python tools/grad_rows.py [--runs N] > profiles/grad_rows.jsonl        (needs a GPU)

--runs N repeats the GPU's backward N times and records the WORST ratio of each statistic (the float atomics reorder
the sums from run to run; the deterministic mode gives the same bits every time)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    import grad_rows as GR
    from gaussiancity_amd import ext
    from oracle import oracle as O
    from test_gpu_parity import _check_forward
    O.build()
    ext.poison_outputs = True   # as the suite runs: the library must write every gradient element itself
    dev = torch.device("cuda:0")
    for name, variant in GR.CASES:
        s = GR.scene(O, name)
        worst = {}
        for _ in range(a.runs):
            state, got = GR.gpu_run(s, variant, dev)
            _check_forward(s.frame, state, s.P, s.use_sh, has_cov3d_state=s.cov3D is None)
            for n in s.names:
                st = GR.row_stats(s.ref[n], got[n])
                w = worst.setdefault(n, st)
                for k in GR.STATS + ("spurious",):
                    w[k] = max(w[k], st[k])
        for n in s.names:
            o, g = s.oracle_stats[n], worst[n]
            print(json.dumps(dict(
                scene=name, variant=variant, tensor=n, rows=o["rows"], runs=a.runs,
                oracle={k: float("%.3e" % o[k]) for k in GR.STATS}, gpu={k: float("%.3e" % g[k]) for k in GR.STATS},
                ratio={k: round(g[k] / (o[k] + GR.ABS / GR.M), 3) for k in GR.STATS},
                within_4x=GR.within(g, o), spurious_rows=g["spurious"])), flush=True)


if __name__ == "__main__":
    main()
