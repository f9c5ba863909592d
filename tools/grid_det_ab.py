"""A/B timing of the hash-grid encoder's two table-gradient paths at the GaussianCity shape: the atomic backward
(gce_backward_t) against the deterministic one (gce_backward_det), in one process, alternating.

  python tools/grid_det_ab.py [--reps 7] [--iters 10] [--points 16384] [--out profiles/grid_det_backward.jsonl]

Shape: D = 5, 16 levels x 8 channels, 2^19 rows per level (268 MB table), 16 384 uniform points, float32, no input
gradient (GaussianCity's points do not require one).  Each path is called into its own preallocated gradient table,
which is not re-zeroed between calls (both paths only add into it), so a call is the backward pass alone; the
deterministic path uses one preallocated workspace.  After a warm-up of both paths: --reps rounds, in each round one
block of --iters atomic calls and one block of --iters deterministic calls between device events; the figure is the
median over the rounds of a block's time per call.  The two results are compared before timing (the project's bar for
this output).  One JSON line per path.  Needs a GPU; there is no CPU path."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiancity_amd import _native_e as E  # noqa: E402
from gaussiancity_amd import grid_encoder as GE  # noqa: E402


def block_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_det_backward.jsonl"))
    a = ap.parse_args()
    if a.reps < 7 or a.iters < 10:
        raise SystemExit("at least 7 blocks of 10 calls")
    if not torch.cuda.is_available():
        raise SystemExit("grid_det_ab needs a GPU")
    dev = torch.device("cuda:0")
    D, L, C, B = 5, 16, 8, a.points
    enc = GE.GridEncoder(D, L, C, 2048).to(dev)
    rows = int(enc.embeddings.shape[0])
    S, H = math.log2(enc.per_level_scale), enc.base_resolution
    g = torch.Generator(device="cpu").manual_seed(2024)
    x = torch.rand(B, D, generator=g).to(dev)
    grad = torch.randn(L, B, C, generator=g).to(dev)
    none = torch.empty(1, device=dev)
    ws_bytes = int(E.lib().gce_backward_det_workspace_bytes(B, D, L, rows))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    tables = {"atomic": torch.zeros_like(enc.embeddings), "deterministic": torch.zeros_like(enc.embeddings)}
    GE.set_deterministic(False)  # ext_backward below is the atomic path whatever the environment says

    def call(path):
        args = (grad, x, enc.embeddings, enc.offsets, tables[path], B, D, C, L, S, H, False, none, none, 0, False)
        if path == "atomic":
            GE.ext_backward(*args)
        else:
            GE.ext_backward_deterministic(*args, workspace=ws)

    for path in tables:  # first calls: code objects load; and the two results agree
        call(path)
    torch.cuda.synchronize()
    ref = tables["atomic"]
    diff = float((tables["deterministic"] - ref).abs().max())
    bar = 1e-5 * max(1.0, float(ref.abs().max()))
    if not diff <= bar:
        raise SystemExit("the two paths disagree: max|d| = %g > %g" % (diff, bar))
    for _ in range(2):
        for path in tables:
            block_ms(lambda: call(path), a.iters)
    times = {path: [] for path in tables}
    for _ in range(a.reps):
        for path in tables:
            times[path].append(block_ms(lambda: call(path), a.iters))
    med = {path: statistics.median(t) for path, t in times.items()}
    n = L * B * (1 << D)
    lines = []
    for path in tables:
        lines.append({"tool": "grid_det_ab", "path": path, "device": torch.cuda.get_device_name(dev), "D": D, "L": L, "C": C,
                      "points": B, "rows": rows, "contributions": n, "reps": a.reps, "iters": a.iters,
                      "ms_per_call_median": round(med[path], 4), "ms_per_call_min": round(min(times[path]), 4),
                      "ms_per_call_max": round(max(times[path]), 4),
                      "ratio_to_atomic": round(med[path] / med["atomic"], 3),
                      "workspace_bytes": ws_bytes if path == "deterministic" else 0,
                      "max_abs_diff_vs_atomic": diff if path == "deterministic" else 0.0})
    out_dir = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(out_dir, exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
