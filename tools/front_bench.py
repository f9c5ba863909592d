"""Timing of the fused front of a PTv3 Block (gaussiancity_amd.front.conv_tail_norm_qkv) against the
five torch ops it replaces, on the same inputs in one process.

  python tools/front_bench.py [--reps 7] [--iters 10] [--warmup 30] [--out profiles/point_front.jsonl]

Shapes: (rows, channels) of the three encoder stages of a 16 384-point frame that the fused kernels hold (16 384 x 32,
4 292 x 64, 1 063 x 128) and stage 0 of an inference-sized frame (262 144 x 32); O = 3 C.
Sides: `fused`, the operator; `torch`, F.linear, F.layer_norm, the add, F.layer_norm and F.linear -- what Block.forward
runs between its sparse convolution and its attention.  Protocol of tools/ffn_bench.py with the sides alternating: --warmup
untimed calls of each side, then --reps rounds in which each side runs one block of --iters calls between device events;
the median block per side.  One JSON line per shape: forward under no_grad and forward + backward in ms per side and their
ratios (torch / fused: above 1 the operator is faster), peak allocator bytes of one forward + backward of each side, and
per side the largest max|got - x64| / max|x64| over feat, qkv and the ten gradients against the same formulation in float64
on the CPU (rows capped at 16 384 for that check).  Needs a GPU; there is no CPU path."""
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

from ffn_bench import peak_bytes, timed_sides  # noqa: E402
from gaussiancity_amd import front  # noqa: E402

SHAPES = [(16384, 32, "stage0 16384 rows C32"), (4292, 64, "stage1 4292 rows C64"), (1063, 128, "stage2 1063 rows C128"),
          (262144, 32, "stage0 inference 262144 rows C32")]
EPS = 1e-5


def torch_ops(x, s, wc, bc, gc, bec, g1, be1, wq, bq):
    C = x.shape[1]
    feat = x + F.layer_norm(F.linear(s, wc, bc), (C,), gc, bec, EPS)
    return feat, F.linear(F.layer_norm(feat, (C,), g1, be1, EPS), wq, bq)


def fused_op(x, s, wc, bc, gc, bec, g1, be1, wq, bq):
    return front.conv_tail_norm_qkv(x, s, wc, bc, gc, bec, EPS, g1, be1, EPS, wq, bq)


def make(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    O = 3 * C
    leaves = [n(rows, C), n(rows, C), n(C, C) / C ** 0.5, 0.1 * n(C), 1 + 0.5 * n(C), 0.1 * n(C), 1 + 0.5 * n(C), 0.1 * n(C),
              n(O, C) / C ** 0.5, 0.1 * n(O)]
    return leaves, n(rows, C), n(rows, O)


def agreement(op, host, dfeat, dqkv, dev, rows):
    """Largest max|got - x64| / max|x64| over feat, qkv and the ten gradients, on the first `rows` rows."""
    def run(fn, device, dtype):
        leaves = [t[:rows].clone() if i < 2 else t.clone() for i, t in enumerate(host)]
        leaves = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in leaves]
        feat, qkv = fn(*leaves)
        torch.autograd.backward([feat, qkv], [dfeat[:rows].to(device=device, dtype=dtype), dqkv[:rows].to(device=device, dtype=dtype)])
        return [feat.detach().double().cpu(), qkv.detach().double().cpu()] + [t.grad.double().cpu() for t in leaves]
    want = run(torch_ops, "cpu", torch.float64)
    return max(float((g - w).abs().max() / w.abs().max()) for g, w in zip(run(op, dev, torch.float32), want))


def bench_shape(dev, rows, C, warmup, reps, iters, label):
    host, dfeat_host, dqkv_host = make(rows, C, rows + C)
    ops = {"fused": fused_op, "torch": torch_ops}
    leaves = {k: [t.to(dev).requires_grad_(True) for t in host] for k in ops}
    grads = [dfeat_host.to(dev), dqkv_host.to(dev)]

    def fwd(k):
        def run():
            with torch.no_grad():
                return ops[k](*leaves[k])
        return run

    def fwdbwd(k):
        def run():
            for t in leaves[k]:
                t.grad = None
            torch.autograd.backward(list(ops[k](*leaves[k])), grads)
        return run

    O = 3 * C
    rec = {"shape": label, "rows": rows, "channels": C, "projected": O, "workgroups": (rows + 63) // 64,
           "flop_fwd": 2.0 * rows * C * (C + O), "bytes_fused_pass": 24 * rows * C, "bytes_torch_ops": 52 * rows * C}
    check = min(rows, 16384)
    for k in ops:
        rec[k + "_max_rel_diff_vs_float64"] = agreement(ops[k], host, dfeat_host, dqkv_host, dev, check)
    f = timed_sides({k: fwd(k) for k in ops}, warmup, reps, iters)
    fb = timed_sides({k: fwdbwd(k) for k in ops}, warmup, reps, iters)
    for k in ops:
        rec[k + "_fwd_ms"], rec[k + "_fwdbwd_ms"] = round(f[k], 4), round(fb[k], 4)
        rec[k + "_peak_bytes"] = peak_bytes(fwdbwd(k), leaves[k])
    rec["fwd_torch_over_fused"] = round(f["torch"] / f["fused"], 2)
    rec["fwdbwd_torch_over_fused"] = round(fb["torch"] / fb["fused"], 2)
    rec["fused_fwd_tflops"] = round(rec["flop_fwd"] / f["fused"] / 1e9, 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=30, help="untimed calls of every side before its timed blocks")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("front_bench needs a GPU")
    dev = torch.device("cuda:0")
    bench_shape(dev, SHAPES[0][0], SHAPES[0][1], 100, 3, 50, "process warm-up, not reported")  # clocks up before the first shape
    lines = []
    for rows, C, label in SHAPES:
        rec = bench_shape(dev, rows, C, a.warmup, a.reps, a.iters, label)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
