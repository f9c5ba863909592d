"""Index plans of the point backbone (include/gcs.h, gaussiancity_amd/point_index.py) at GaussianCity's shapes: 16 384
points (a training frame) and 150 000 (an inference frame), 57 batches, depth 8, patch 1024.  Three items per shape:

  serialize_cord     serialize() for ("cord",), GaussianCity's own configuration
  serialize_curves   serialize() for PTv3's default ("z", "z-trans", "hilbert", "hilbert-trans")
  patch_plan         patch_plan(offset, 1024)

Each is timed in ONE process in alternation with a torch-ops formulation of the same steps.  That formulation is THIS
TOOL'S OWN, not upstream's text: integer tensors instead of upstream's [n, 3, depth] bit tensors and table rebuilds (so
it is the cheaper torch way to get the codes, and the ratio against upstream's methods would be larger), torch.sort
(stable) and a scatter for the inverse; for the plan, the per-batch loop with its device-scalar comparisons and slices
is KEPT, because that loop is what the library replaces.  Host wall time per call around blocks of calls that end in a
synchronise, median over the rounds; the two sides' results are compared bit for bit first.  Appends one JSON line.
    python tools/point_index_bench.py --out profiles/point_index.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussiancity_amd import point_index as PI  # noqa: E402

CURVES = ("z", "z-trans", "hilbert", "hilbert-trans")


def _interleave(x, y, z, depth):
    key = torch.zeros_like(x)
    for i in range(depth):
        key = key | ((x >> i) & 1) << (3 * i + 2) | ((y >> i) & 1) << (3 * i + 1) | ((z >> i) & 1) << (3 * i)
    return key


def _hilbert(x, y, z, depth):
    X = [x, y, z]
    Q = 1 << (depth - 1)
    while Q > 1:
        P = Q - 1
        for i in range(3):
            on = (X[i] & Q) != 0
            t = torch.where(on, 0, (X[0] ^ X[i]) & P)
            X[0] = torch.where(on, X[0] ^ P, X[0] ^ t)
            if i:
                X[i] = X[i] ^ t
        Q >>= 1
    h = _interleave(X[0], X[1], X[2], depth)
    for s in (1, 2, 4, 8, 16, 32):
        h = h ^ (h >> s)
    return h


def torch_serialize(grid, batch, depth, orders, grid_size=0.01):
    g = grid.long()
    m = (1 << depth) - 1
    x, y, z = g[:, 0] & m, g[:, 1] & m, g[:, 2] & m
    rows = []
    for name in orders:
        if name == "cord":
            c = (g[:, 0] / grid_size ** 2 + g[:, 1] / grid_size + g[:, 2]).long()
        elif name == "z":
            c = _interleave(x, y, z, depth)
        elif name == "z-trans":
            c = _interleave(y, x, z, depth)
        elif name == "hilbert":
            c = _hilbert(x, y, z, depth)
        else:
            c = _hilbert(y, x, z, depth)
        rows.append(batch << depth * 3 | c)
    code = torch.stack(rows)
    order = torch.sort(code, dim=1, stable=True).indices
    inverse = torch.zeros_like(order).scatter_(1, order, torch.arange(code.shape[1], device=code.device).repeat(len(rows), 1))
    return code, order, inverse


def torch_patch_plan(offset, P):
    count = torch.diff(offset, prepend=offset.new_zeros(1))
    count_pad = torch.where(count > P, (count + P - 1) // P * P, count)
    start = torch.nn.functional.pad(offset, (1, 0))
    start_pad = torch.nn.functional.pad(torch.cumsum(count_pad, 0), (1, 0))
    pad = torch.arange(int(start_pad[-1]), device=offset.device)
    unpad = torch.arange(int(start[-1]), device=offset.device)
    cu = []
    for i in range(len(offset)):   # the per-batch loop: every comparison and slice bound below is a device scalar
        shift = start_pad[i] - start[i]
        unpad[start[i]:start[i + 1]] += shift
        if count[i] != count_pad[i]:
            tail = start_pad[i] + count[i]
            pad[tail:start_pad[i + 1]] = pad[tail - P:start_pad[i + 1] - P].clone()
        pad[start_pad[i]:start_pad[i + 1]] -= shift
        cu.append(torch.arange(start_pad[i], start_pad[i + 1], step=P, dtype=torch.int32, device=offset.device))
    return pad, unpad, torch.nn.functional.pad(torch.concat(cu), (0, 1), value=int(start_pad[-1]))


def alternate(a, b, rounds, reps):
    """ms per call of a and of b: `rounds` rounds of (reps x a, synchronise, reps x b, synchronise), medians."""
    ta, tb = [], []
    for fn in (a, b, a, b):
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for fn, acc in ((a, ta), (b, tb)):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            acc.append(1e3 * (time.perf_counter() - t0) / reps)
    return statistics.median(ta), statistics.median(tb), ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[16384, 150000])
    ap.add_argument("--batches", type=int, default=57)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--patch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_index.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("point_index_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    items, exact = [], True
    for n in args.points:
        rng = np.random.default_rng(n)
        counts = rng.multinomial(n - args.batches, np.ones(args.batches) / args.batches) + 1
        offset = torch.from_numpy(np.cumsum(counts)).to(dev)
        batch = torch.from_numpy(np.repeat(np.arange(args.batches), counts)).to(dev)
        grid = torch.from_numpy(rng.integers(0, 1 << args.depth, (n, 3)).astype(np.int32)).to(dev)
        for item, orders in (("serialize_cord", ("cord",)), ("serialize_curves", CURVES)):
            lib = lambda: PI.serialize(grid, batch, args.depth, orders, 0.01, args.batches)  # noqa: E731
            ops = lambda: torch_serialize(grid, batch, args.depth, orders)  # noqa: E731
            got, want = lib(), ops()
            same = [bool(torch.equal(g, w)) for g, w in zip(got, want)]
            note = None
            if item == "serialize_cord" and not same[0]:
                # torch's device kernel may multiply by the reciprocal where the library divides: count it,
                # and compare order and inverse on the library's own codes
                note = "cord codes differ from torch's on-device expression in %d of %d elements" % (int((got[0] != want[0]).sum()), n)
                o = torch.sort(got[0], dim=1, stable=True).indices
                same = [True, bool(torch.equal(got[1], o)), bool(torch.equal(torch.gather(got[2], 1, o), torch.arange(n, device=dev)[None]))]
            exact = exact and all(same)
            la, lb, ra, rb = alternate(lib, ops, args.rounds, args.reps)
            items.append({"item": item, "points": n, "orders": list(orders), "library_ms": round(la, 4), "torch_ops_ms": round(lb, 4),
                          "torch_ops_over_library": round(lb / la, 2), "library_ms_rounds": [round(v, 4) for v in ra],
                          "torch_ops_ms_rounds": [round(v, 4) for v in rb], "equal_bit_for_bit": all(same), "note": note})
        lib = lambda: PI.patch_plan(offset, args.patch)  # noqa: E731
        ops = lambda: torch_patch_plan(offset, args.patch)  # noqa: E731
        same = all(bool(torch.equal(g, w)) and g.dtype == w.dtype for g, w in zip(lib(), ops()))
        exact = exact and same
        la, lb, ra, rb = alternate(lib, ops, args.rounds, max(1, args.reps // 4))
        items.append({"item": "patch_plan", "points": n, "patch": args.patch, "library_ms": round(la, 4), "torch_ops_ms": round(lb, 4),
                      "torch_ops_over_library": round(lb / la, 2), "library_ms_rounds": [round(v, 4) for v in ra],
                      "torch_ops_ms_rounds": [round(v, 4) for v in rb], "equal_bit_for_bit": same, "note": None})
    rec = {"tool": "tools/point_index_bench.py", "device": torch.cuda.get_device_name(0),
           "shape": {"batches": args.batches, "depth": args.depth, "patch": args.patch},
           "timing": "host wall ms per call, blocks of calls ending in a synchronise, library and torch-ops formulation "
                     "alternating in one process, median of %d rounds" % args.rounds,
           "torch_ops": "this tool's own integer-tensor formulation (cheaper than upstream's bit tensors); the plan keeps the per-batch loop",
           "items": items}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))
    if not exact:
        raise SystemExit("library and torch-ops results differ")


if __name__ == "__main__":
    main()
