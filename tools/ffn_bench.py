"""Timing of the fused feed-forward third of a PTv3 Block (gaussiancity_amd.ffn.layernorm_mlp_residual, DESIGN.md section
18) against the torch ops it replaces, on the same inputs in one process.

  python tools/ffn_bench.py [--reps 7] [--iters 10] [--warmup 30] [--inference-n 262144] [--out profiles/point_ffn.jsonl]
  python tools/ffn_bench.py --split [--shapes 1063x128,4400x256] [--out profiles/point_ffn_split.jsonl]

Shapes: (rows, channels) of the five encoder stages of a 16 384-point frame as PTv3 pools them (16 384 x 32, 4 292 x 64,
1 063 x 128, 271 x 256, 73 x 512; hidden width 4 C) and stage 0 of an inference-sized frame.  Stages wider than
ffn.max_channels() are what point_ffn hands to the module's own method: they are listed with the torch side only.
Sides: `fused`, the operator; `torch`, F.layer_norm, F.linear, F.gelu, F.linear and the add -- Block.forward's tail with
DropPath at 0; with --split also `split`, the operator with split=True (gcm_ffn_split_*, C up to 512), on SPLIT_SHAPES, with
the library's plan for the shape in the record.  Protocol of tools/attn_bench.py with the sides alternating: --warmup untimed calls of each side, then
--reps rounds in which each side runs one block of --iters calls between device events; the median block per side.
One JSON line per shape: forward under no_grad and forward + backward in ms per side and their ratios (torch / fused:
above 1 the operator is faster), peak allocator bytes of one forward + backward of each side, and per side the largest
max|got - x64| / max|x64| over y and the seven gradients against the same formulation in float64 on the CPU (rows capped at
16 384 for that check).  Needs a GPU; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiancity_amd import ffn  # noqa: E402

STAGES = [(16384, 32), (4292, 64), (1063, 128), (271, 256), (73, 512)]
EPS = 1e-5
NAMES = ("x", "ln_w", "ln_b", "w1", "b1", "w2", "b2")


def torch_ops(x, ln_w, ln_b, w1, b1, w2, b2):
    return x + F.linear(F.gelu(F.linear(F.layer_norm(x, (x.shape[1],), ln_w, ln_b, EPS), w1, b1)), w2, b2)


def fused_op(x, ln_w, ln_b, w1, b1, w2, b2):
    return ffn.layernorm_mlp_residual(x, ln_w, ln_b, EPS, w1, b1, w2, b2)


def split_op(x, ln_w, ln_b, w1, b1, w2, b2):
    return ffn.layernorm_mlp_residual(x, ln_w, ln_b, EPS, w1, b1, w2, b2, split=True)


# --split: the shapes of the split operator's write-up.  The last two are the wide stages of an
# inference-sized frame estimated from the / 3.9 per stage of the training shapes, not counted on a real frame.
SPLIT_SHAPES = [(271, 256), (73, 512), (1063, 128), (16384, 32), (4400, 256), (1100, 512)]


def timed_sides(sides, warmup, reps, iters):
    """{side: median ms per call}: every side warmed up, then `reps` rounds of one block of `iters` calls per side."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / iters)
    return {k: statistics.median(v) for k, v in out.items()}


def peak_bytes(fn, leaves):
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def make(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    Hd = 4 * C
    return [n(rows, C), 1 + 0.5 * n(C), 0.1 * n(C), n(Hd, C) / C ** 0.5, 0.1 * n(Hd), n(C, Hd) / Hd ** 0.5, 0.1 * n(C)], n(rows, C)


def agreement(op, host, dy, dev, rows):
    """Largest max|got - x64| / max|x64| over y and the seven gradients, on the first `rows` rows."""
    def run(fn, device, dtype):
        leaves = [t[:rows].clone() if i == 0 else t.clone() for i, t in enumerate(host)]
        leaves = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in leaves]
        y = fn(*leaves)
        y.backward(dy[:rows].to(device=device, dtype=dtype))
        return [y.detach().double().cpu()] + [t.grad.double().cpu() for t in leaves]
    want = run(torch_ops, "cpu", torch.float64)
    return max(float((g - w).abs().max() / w.abs().max()) for g, w in zip(run(op, dev, torch.float32), want))


def bench_shape(dev, rows, C, warmup, reps, iters, label, split=False):
    host, dy_host = make(rows, C, rows + C)
    fusable = C <= ffn.max_channels()
    ops = {"fused": fused_op, "torch": torch_ops} if fusable else {"torch": torch_ops}
    if split:
        ops["split"] = split_op
    leaves = {k: [t.to(dev).requires_grad_(True) for t in host] for k in ops}
    dy = dy_host.to(dev)

    def fwd(k):
        def run():
            with torch.no_grad():
                return ops[k](*leaves[k])
        return run

    def fwdbwd(k):
        def run():
            for t in leaves[k]:
                t.grad = None
            ops[k](*leaves[k]).backward(dy)
        return run

    rec = {"shape": label, "rows": rows, "channels": C, "hidden": 4 * C, "fused": fusable,
           "flop_fwd": 4.0 * rows * C * 4 * C, "bytes_fused_pass": 8 * rows * C, "bytes_torch_ops": 92 * rows * C}
    check = min(rows, 16384)
    for k in ops:
        rec[k + "_max_rel_diff_vs_float64"] = agreement(ops[k], host, dy_host, dev, check)
    f = timed_sides({k: fwd(k) for k in ops}, warmup, reps, iters)
    fb = timed_sides({k: fwdbwd(k) for k in ops}, warmup, reps, iters)
    for k in ops:
        rec[k + "_fwd_ms"], rec[k + "_fwdbwd_ms"] = round(f[k], 4), round(fb[k], 4)
        rec[k + "_peak_bytes"] = peak_bytes(fwdbwd(k), leaves[k])
    if fusable:
        rec["fwd_torch_over_fused"] = round(f["torch"] / f["fused"], 2)
        rec["fwdbwd_torch_over_fused"] = round(fb["torch"] / fb["fused"], 2)
        rec["fused_fwd_tflops"] = round(rec["flop_fwd"] / f["fused"] / 1e9, 3)
    if split:
        rec["split_plan"] = ffn.split_plan(rows, C, 4 * C)
        rec["fwd_torch_over_split"] = round(f["torch"] / f["split"], 2)
        rec["fwdbwd_torch_over_split"] = round(fb["torch"] / fb["split"], 2)
        if fusable:
            rec["fwd_fused_over_split"] = round(f["fused"] / f["split"], 2)
            rec["fwdbwd_fused_over_split"] = round(fb["fused"] / fb["split"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=30, help="untimed calls of every side before its timed blocks")
    ap.add_argument("--inference-n", type=int, default=262144)
    ap.add_argument("--out", default=None)
    ap.add_argument("--split", action="store_true",
                    help="SPLIT_SHAPES with the split operator (split=True) as a third side, instead of the stages")
    ap.add_argument("--shapes", default=None, help="with --split: rows x channels pairs instead, as 1063x128,4400x256")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ffn_bench needs a GPU")
    dev = torch.device("cuda:0")
    cases = [(rows, C, "stage%d %d rows C%d" % (i, rows, C)) for i, (rows, C) in enumerate(STAGES)]
    if a.split:
        pairs = [tuple(int(v) for v in p.split("x")) for p in a.shapes.split(",")] if a.shapes else SPLIT_SHAPES
        cases = [(rows, C, "%d rows C%d" % (rows, C)) for rows, C in pairs]
    elif a.inference_n:
        cases.append((a.inference_n, 32, "stage0 inference %d rows C32" % a.inference_n))
    bench_shape(dev, STAGES[0][0], STAGES[0][1], 100, 3, 50, "process warm-up, not reported")  # clocks up before the first shape
    lines = []
    for rows, C, label in cases:
        rec = bench_shape(dev, rows, C, a.warmup, a.reps, a.iters, label, a.split)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
