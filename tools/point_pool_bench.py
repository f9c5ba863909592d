"""SerializedPooling / SerializedUnpooling over the library (include/gcs.h, gaussiancity_amd/point_pool.py) at the four
encoder stages of a 150 000-point, 57-batch frame at depth 8 (channels 32 -> 64, 64 -> 128, 128 -> 256, 256 -> 512,
stride 2, float32; every batch is a sloped surface three voxels thick inside a box of 48 x 48 columns, so that the first
stage's clusters hold a few rows each), for GaussianCity's own order ("cord",) and for PTv3's four curve orders.  Three items per stage:

  plan        pool_plan(code, 1) against upstream's steps: torch.unique, torch.sort, cumsum, the gathers, the sort of the
              pooled codes and the scatter for its inverse
  pooling     forward + backward of the data half for a given plan: the `max` reduce of the projected features [n, Cout]
              and the `mean` reduce of coord [n, 3]; the projection itself is the same product on both sides and is not
              timed
  unpooling   forward + backward of parent [n, Cin] + child[cluster]

The YARDSTICK is upstream's text in torch ops with this library's existing segment_csr (`segment_csr(x[indices], idx_ptr)`,
`a + b[inverse]`, autograd's index_put in the backward): what the backbone ran before the rebinding.  Both sides are timed
in ONE process in alternation, host wall time per call around blocks of calls that end in a synchronise, median over the
rounds; the two sides' results are compared first (bit for bit, except the yardstick's own unpooling gradient, whose
index_put sums in another order).  Appends one JSON line.
    python tools/point_pool_bench.py --out profiles/point_pool.jsonl
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
from gaussiancity_amd import point_pool as PP  # noqa: E402
from gaussiancity_amd.sparse import segment_csr  # noqa: E402

CURVES = ("z", "z-trans", "hilbert", "hilbert-trans")
CHANNELS = ((32, 64), (64, 128), (128, 256), (256, 512))


def torch_plan(code, depth):
    """Upstream's steps (models/pt_v3.py, SerializedPooling.forward), with stable sorts so that the results compare."""
    code = code >> depth * 3
    _, cluster, counts = torch.unique(code[0], sorted=True, return_inverse=True, return_counts=True)
    indices = torch.sort(cluster, stable=True).indices
    idx_ptr = torch.cat([counts.new_zeros(1), torch.cumsum(counts, dim=0)])
    head = indices[idx_ptr[:-1]]
    code = code[:, head]
    order = torch.sort(code, dim=1, stable=True).indices
    inverse = torch.zeros_like(order).scatter_(1, order, torch.arange(code.shape[1], device=code.device).repeat(code.shape[0], 1))
    return cluster, indices, idx_ptr, head, code, order, inverse


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
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--batches", type=int, default=57)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_pool.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("point_pool_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    n0 = args.points
    rng = np.random.default_rng(n0)
    counts = rng.multinomial(n0 - args.batches, np.ones(args.batches) / args.batches) + 1
    batch0 = torch.from_numpy(np.repeat(np.arange(args.batches), counts)).to(dev)
    # every batch (an instance) is a surface inside its own box of 48 x 48 columns: z within three layers of a slope, so that
    # a cell of 2 x 2 x 2 voxels holds a few rows, as a frame's clusters do (1...8 rows), and some voxels hold several
    origin = np.repeat(rng.integers(0, (1 << args.depth) - 48, (args.batches, 2)), counts, axis=0)
    xy = origin + rng.integers(0, 48, (n0, 2))
    z = ((xy[:, 0] + xy[:, 1]) // 4 + rng.integers(0, 3, n0)) & ((1 << args.depth) - 1)
    grid0 = torch.from_numpy(np.concatenate([xy, z[:, None]], 1).astype(np.int32)).to(dev)
    items, exact = [], True

    def record(item, stage, orders, n, s, width, same, la, lb, ra, rb, note=None):
        items.append({"item": item, "stage": stage, "orders": list(orders), "rows": n, "clusters": s, "width": width,
                      "library_ms": round(la, 4), "yardstick_ms": round(lb, 4), "yardstick_over_library": round(lb / la, 2),
                      "library_ms_rounds": [round(v, 4) for v in ra], "yardstick_ms_rounds": [round(v, 4) for v in rb],
                      "equal_bit_for_bit": bool(same), "note": note})

    for orders in (("cord",), CURVES):
        grid, batch = grid0, batch0
        code = PI.serialize(grid, batch, args.depth, orders, 0.01, args.batches)[0]
        for stage, (cin, cout) in enumerate(CHANNELS, 1):
            n = int(code.shape[1])
            plan = PP.pool_plan(code, 1)
            want = torch_plan(code, 1)
            same = all(bool(torch.equal(getattr(plan, f), w)) for f, w in zip(PP.FIELDS, want))
            exact = exact and same
            la, lb, ra, rb = alternate(lambda: PP.pool_plan(code, 1), lambda: torch_plan(code, 1), args.rounds, args.reps)
            record("plan", stage, orders, n, plan.s, None, same, la, lb, ra, rb)

            g = torch.Generator().manual_seed(stage)
            y = torch.randn(n, cout, generator=g).to(dev).requires_grad_(True)
            coord = torch.rand(n, 3, generator=g).to(dev)
            dout = torch.randn(plan.s, cout, generator=g).to(dev)

            def lib_pool():
                y.grad = None
                out = PP.pooled_reduce(y, plan, "max")
                c = PP.pooled_reduce(coord, plan, "mean")
                out.backward(dout)
                return out.detach(), c, y.grad

            def ops_pool():
                y.grad = None
                out = segment_csr(y[plan.indices], plan.idx_ptr, reduce="max")
                c = segment_csr(coord[plan.indices], plan.idx_ptr, reduce="mean")
                out.backward(dout)
                return out.detach(), c, y.grad

            same = all(bool(torch.equal(a, b)) for a, b in zip(lib_pool(), ops_pool()))
            exact = exact and same
            la, lb, ra, rb = alternate(lib_pool, ops_pool, args.rounds, args.reps)
            record("pooling", stage, orders, n, plan.s, cout, same, la, lb, ra, rb)

            a = torch.randn(n, cin, generator=g).to(dev).requires_grad_(True)
            b = torch.randn(plan.s, cin, generator=g).to(dev).requires_grad_(True)
            up = torch.randn(n, cin, generator=g).to(dev)

            def lib_unpool():
                a.grad = b.grad = None
                out = PP.unpool_add(a, b, plan)
                out.backward(up)
                return out.detach(), a.grad, b.grad

            def ops_unpool():
                a.grad = b.grad = None
                out = a + b[plan.cluster]
                out.backward(up)
                return out.detach(), a.grad, b.grad

            got, ref = lib_unpool(), ops_unpool()
            same = bool(torch.equal(got[0], ref[0])) and bool(torch.equal(got[1], ref[1]))
            exact = exact and same and bool(torch.allclose(got[2], ref[2], rtol=1e-4, atol=1e-4))
            note = "d_child differs from the yardstick's index_put sum by at most %.2e (another summation order)" % float(
                (got[2] - ref[2]).abs().max())
            la, lb, ra, rb = alternate(lib_unpool, ops_unpool, args.rounds, args.reps)
            record("unpooling", stage, orders, n, plan.s, cin, same, la, lb, ra, rb, note)

            grid, batch, code = grid[plan.head] >> 1, batch[plan.head], plan.code
    rec = {"tool": "tools/point_pool_bench.py", "device": torch.cuda.get_device_name(0),
           "shape": {"points": n0, "batches": args.batches, "depth": args.depth, "stride": 2, "dtype": "float32"},
           "timing": "host wall ms per call, blocks of %d calls ending in a synchronise, library and yardstick alternating in one "
                     "process, median of %d rounds" % (args.reps, args.rounds),
           "yardstick": "upstream's steps in torch ops with this library's segment_csr: segment_csr(x[indices], idx_ptr), "
                        "a + b[inverse], autograd's index_put backward; sorts stable so that the plans compare",
           "items": items}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))
    if not exact:
        raise SystemExit("library and yardstick results differ")


if __name__ == "__main__":
    main()
