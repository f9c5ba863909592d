"""Timing of the fused middle of a PTv3 Block (gaussiancity_amd.mid: slot_plan + gather_rows + proj_residual, DESIGN.md
section 20) against the torch ops it replaces, on the same inputs in one process; the attention between the gather and
the projection is excluded on both sides (its output is a leaf).

  timeout -k 10 900 python tools/mid_bench.py [--reps 7] [--iters 10] [--warmup 30] [--out profiles/point_mid.jsonl]

Shapes: section 19's four (16 384 x 32, 4 292 x 64, 1 063 x 128, 262 144 x 32), each as two batch elements of 3 / 5 and
2 / 5 of the rows with a seeded serialization order, padded as get_padding_and_inverse pads them for --patch (1024), so that
duplicate slots exist; qkv is 3 C wide.
Sides: `fused`, the plan and the two operators; `torch`, qkv[order], a[inverse], F.linear, the mask multiply (forward +
backward only: under no_grad the Block is in eval mode and there is no mask) and the add.  Protocol of tools/front_bench.py:
--warmup untimed calls of each side, then --reps rounds in which each side runs one block of --iters calls between device
events; the median block per side.  One JSON line per shape: forward under no_grad and forward + backward in ms per side and
their ratios (torch / fused: above 1 the operator is faster), and per side the largest max|got - x64| / max|x64| over the
outputs and gradients against float64 on the CPU (rows capped at 16 384).  One more line, `index_put backwards alone`:
per shape the time of the two sort-based index_put_(accumulate=True) that torch's backward runs for qkv[order] and
a[inverse], beside mid's gradient of the first (the second is the scatter inside its row kernel) and the share of torch's
backward (forward + backward minus forward) they are.
Needs a GPU; there is no CPU path."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from ffn_bench import timed_sides  # noqa: E402
from front_bench import SHAPES  # noqa: E402
from gaussiancity_amd import mid  # noqa: E402

KEEP = 0.7


def index_pair(rows, patch, seed):
    """(order [T], inverse [N]) of two batch elements as SerializedAttention's non-flash branch builds them: the patch size
    is the smaller element's count, capped; an element above it that is no multiple fills its last patch from the one before."""
    g = torch.Generator().manual_seed(seed)
    counts = (rows * 3 // 5, rows - rows * 3 // 5)
    K = min(min(counts), patch)
    pad, unpad, start, pstart = [], [], 0, 0
    for n in counts:
        own = list(range(n))
        if n > K and n % K:
            m, r = n // K, n % K
            own += list(range((m - 1) * K + r, m * K))
        pad += [start + j for j in own]
        unpad += [pstart + j for j in range(n)]
        start, pstart = start + n, pstart + len(own)
    serial = torch.cat([torch.randperm(n, generator=g) + o for n, o in zip(counts, (0, counts[0]))])
    inv = torch.empty_like(serial)
    inv[serial] = torch.arange(rows)
    return serial[torch.tensor(pad)], torch.tensor(unpad)[inv]


def torch_ops(qkv, a, x, wp, bp, order, inverse, r):
    p = F.linear(a[inverse], wp, bp)
    return qkv[order], x + (p if r is None else p * r)


def fused_op(qkv, a, x, wp, bp, order, inverse, r):
    extra = mid.slot_plan(order, inverse) if torch.is_grad_enabled() else None  # as point_mid.middle: the gradients read it
    return mid.gather_rows(qkv, order, inverse, extra), mid.proj_residual(a, inverse, extra, x, wp, bp, r)


def make(rows, T, C, seed):
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    leaves = [n(rows, 3 * C), n(T, C), n(rows, C), n(C, C) / C ** 0.5, 0.1 * n(C)]
    r = (torch.rand(rows, 1, generator=g) < KEEP).float() / KEEP
    return leaves, n(T, 3 * C), n(rows, C), r


def agreement(op, host, grads, r, patch, dev, rows, seed):
    """Largest max|got - x64| / max|x64| over both outputs and the five gradients, on the first `rows` rows."""
    order, inverse = index_pair(rows, patch, seed)
    T = order.shape[0]

    def run(fn, device, dtype):
        cut = (rows, T, rows)
        leaves = [t[:cut[i]].clone() if i < 3 else t.clone() for i, t in enumerate(host)]
        leaves = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in leaves]
        outs = fn(*leaves, order.to(device), inverse.to(device), r[:rows].to(device=device, dtype=dtype))
        torch.autograd.backward(list(outs), [grads[0][:T].to(device=device, dtype=dtype), grads[1][:rows].to(device=device, dtype=dtype)])
        return [o.detach().double().cpu() for o in outs] + [t.grad.double().cpu() for t in leaves]
    want = run(torch_ops, "cpu", torch.float64)
    return max(float((g - w).abs().max() / w.abs().max()) for g, w in zip(run(op, dev, torch.float32), want))


def bench_shape(dev, rows, C, patch, warmup, reps, iters, label):
    order_host, inverse_host = index_pair(rows, patch, rows + C)
    T = order_host.shape[0]
    host, dpacked_host, dy_host, r_host = make(rows, T, C, rows + C)
    ops = {"fused": fused_op, "torch": torch_ops}
    leaves = {k: [t.to(dev).requires_grad_(True) for t in host] for k in ops}
    order, inverse, r = order_host.to(dev), inverse_host.to(dev), r_host.to(dev)
    grads = [dpacked_host.to(dev), dy_host.to(dev)]

    def fwd(k):
        def run():
            with torch.no_grad():
                return ops[k](*leaves[k], order, inverse, None)
        return run

    def fwdbwd(k):
        def run():
            for t in leaves[k]:
                t.grad = None
            torch.autograd.backward(list(ops[k](*leaves[k], order, inverse, r)), grads)
        return run

    rec = {"shape": label, "rows": rows, "slots": T, "duplicate_slots": T - rows, "channels": C, "workgroups": (rows + 63) // 64,
           "bytes_fused_pass": 12 * rows * C, "bytes_torch_ops_eval": 28 * rows * C, "bytes_torch_ops_training": 40 * rows * C}
    check = min(rows, 16384)
    for k in ops:
        rec[k + "_max_rel_diff_vs_float64"] = agreement(ops[k], host, (dpacked_host, dy_host), r_host, patch, dev, check, rows + C)
    f = timed_sides({k: fwd(k) for k in ops}, warmup, reps, iters)
    fb = timed_sides({k: fwdbwd(k) for k in ops}, warmup, reps, iters)
    for k in ops:
        rec[k + "_fwd_ms"], rec[k + "_fwdbwd_ms"] = round(f[k], 4), round(fb[k], 4)
    rec["fwd_torch_over_fused"] = round(f["torch"] / f["fused"], 2)
    rec["fwdbwd_torch_over_fused"] = round(fb["torch"] / fb["fused"], 2)

    # the two gather gradients alone: torch's sort-based index_put against mid's gathered sum
    extra = mid.slot_plan(order, inverse)
    da = torch.randn(rows, C, device=dev)

    def index_puts():
        torch.zeros(rows, 3 * C, device=dev).index_put_((order,), grads[0], accumulate=True)
        torch.zeros(T, C, device=dev).index_put_((inverse,), da, accumulate=True)

    q = leaves["fused"][0]
    packed = mid.gather_rows(q, order, inverse, extra)

    def gathered():
        torch.autograd.grad(packed, q, grads[0], retain_graph=True)
    ip = timed_sides({"torch": index_puts, "fused": gathered}, warmup, reps, iters)
    alone = {"index_put_ms": round(ip["torch"], 4), "gather_backward_ms": round(ip["fused"], 4),
             "share_of_torch_backward": round(ip["torch"] / max(fb["torch"] - f["torch"], 1e-9), 2)}
    return rec, alone


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=30, help="untimed calls of every side before its timed blocks")
    ap.add_argument("--patch", type=int, default=1024, help="patch_size_max of the attention")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mid_bench needs a GPU")
    dev = torch.device("cuda:0")
    bench_shape(dev, SHAPES[0][0], SHAPES[0][1], a.patch, 100, 3, 50, "process warm-up, not reported")  # clocks up first
    lines, alone = [], {"shape": "index_put backwards alone"}
    for rows, C, label in SHAPES:
        rec, alone[label] = bench_shape(dev, rows, C, a.patch, a.warmup, a.reps, a.iters, label)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    print(json.dumps(alone), flush=True)
    lines.append(alone)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
