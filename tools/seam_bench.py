"""Timing of the fused stage seam (gaussiancity_amd.seam.linear_bn_gelu) against the torch ops it
replaces (F.linear, F.batch_norm, F.gelu), on the same inputs in one process.

  timeout -k 10 900 python tools/seam_bench.py [--reps 7] [--iters 10] [--warmup 30] [--out profiles/point_seam.jsonl]

Shapes: the backbone's seams -- (16 384, 32 -> 64), (4 292, 64 -> 64), (1 063, 128 -> 128), (300, 256 -> 256),
(300, 512 -> 256), (16 384, 32 with no product: the stem's tail), (262 144, 32 -> 64).
Sides: `fused`, one call of the operator; `torch`, the three ops with the same buffers.  Protocol of tools/mid_bench.py:
--warmup untimed calls of each side, then --reps rounds in which each side runs one block of --iters calls between device
events; the median block per side.  One JSON line per shape: forward under no_grad in eval mode and forward + backward in
training mode in ms per side and their ratios (torch / fused: above 1 the operator is faster), and per side the largest
max|got - x64| / max|x64| over the output and the gradients against float64 on the CPU (rows capped at 16 384), compared
before anything is timed.
One more item, a whole PTv3 forward + backward in training mode with the six installs (point_attention, point_pool,
point_front, point_mid, point_ffn, point_seam) against none, on tools/ptv3_stand_in.py's backbone (its sparse convolutions
are a Linear on the features and its serialization a z-order code in torch ops, on both sides): --model-widths (config.py's
encoder widths), --model-orders (1: GaussianCity's single order), --model-patch, and tools/point_pool_bench.py's
sloped-surface frame of --model-points in --model-batches at --model-depth.  Host wall ms per pass around blocks of
--model-iters passes that end in a synchronise, the sides alternating, the median of --reps rounds; the two sides' output
and input gradient are compared first.
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
from gaussiancity_amd import seam  # noqa: E402

EPS, MOMENTUM = 1e-3, 0.01
SHAPES = ((16384, 32, 64, True, "16 384 x 32 -> 64"), (4292, 64, 64, True, "4 292 x 64 -> 64"),
          (1063, 128, 128, True, "1 063 x 128 -> 128"), (300, 256, 256, True, "300 x 256 -> 256"),
          (300, 512, 256, True, "300 x 512 -> 256"), (16384, 32, 32, False, "16 384 x 32, no product"),
          (262144, 32, 64, True, "262 144 x 32 -> 64"))


def torch_ops(x, w, b, g, h, rm, rv, nbt, training):
    z = x if w is None else F.linear(x, w, b)
    if training:
        nbt += 1  # BatchNorm1d's own line
    return F.gelu(F.batch_norm(z, rm, rv, g, h, training, MOMENTUM, EPS))


def fused_op(x, w, b, g, h, rm, rv, nbt, training):
    return seam.linear_bn_gelu(x, w, b, g, h, rm, rv, nbt, training=training, momentum=MOMENTUM, eps=EPS)


def make(rows, I, O, product, seed):
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    leaves = [n(rows, I), n(O, I) / I ** 0.5 if product else None, 0.1 * n(O) if product else None, 1 + 0.5 * n(O), 0.1 * n(O)]
    return leaves, [0.3 * n(O), 0.5 + torch.rand(O, generator=g), torch.tensor(0)], n(rows, O)


def agreement(op, host, bufs, dy, dev, rows, training):
    """Largest max|got - x64| / max|x64| over the output and the gradients, on the first `rows` rows."""
    def run(fn, device, dtype):
        leaves = [None if t is None else (t[:rows] if i == 0 else t).clone().to(device=device, dtype=dtype).requires_grad_(True)
                  for i, t in enumerate(host)]
        b = [bufs[0].clone().to(device=device, dtype=dtype), bufs[1].clone().to(device=device, dtype=dtype), bufs[2].clone().to(device)]
        y = fn(*leaves, *b, training)
        y.backward(dy[:rows].to(device=device, dtype=dtype))
        return [y.detach().double().cpu()] + [t.grad.double().cpu() for t in leaves if t is not None]
    want, got = run(torch_ops, "cpu", torch.float64), run(op, dev, torch.float32)
    # (a bias in front of batch statistics has the gradient 0: it is measured against its weight's maximum)
    scale = [w.abs().max() for w in want]
    if training and host[1] is not None:
        scale[3] = scale[2]
    return max(float((g - w).abs().max() / s) for g, w, s in zip(got, want, scale))


def bench_shape(dev, rows, I, O, product, warmup, reps, iters, label):
    host, bufs_host, dy_host = make(rows, I, O, product, rows + I + O)
    ops = {"fused": fused_op, "torch": torch_ops}
    leaves = {k: [None if t is None else t.to(dev).requires_grad_(True) for t in host] for k in ops}
    bufs = {k: [t.clone().to(dev) for t in bufs_host] for k in ops}
    dy = dy_host.to(dev)

    def fwd(k):
        def run():
            with torch.no_grad():
                return ops[k](*leaves[k], *bufs[k], False)
        return run

    def fwdbwd(k):
        def run():
            for t in leaves[k]:
                if t is not None:
                    t.grad = None
            ops[k](*leaves[k], *bufs[k], True).backward(dy)
        return run

    rec = {"shape": label, "rows": rows, "inputs": I, "outputs": O, "product": product, "workgroups": (rows + 63) // 64,
           "bytes_fused_eval": 4 * rows * I + 4 * rows * O, "bytes_torch_ops_eval": 4 * rows * I + 20 * rows * O}
    check = min(rows, 16384)
    for k in ops:
        rec[k + "_eval_max_rel_diff_vs_float64"] = agreement(ops[k], host, bufs_host, dy_host, dev, check, False)
        rec[k + "_train_max_rel_diff_vs_float64"] = agreement(ops[k], host, bufs_host, dy_host, dev, check, True)
    f = timed_sides({k: fwd(k) for k in ops}, warmup, reps, iters)
    fb = timed_sides({k: fwdbwd(k) for k in ops}, warmup, reps, iters)
    for k in ops:
        rec[k + "_eval_fwd_ms"], rec[k + "_train_fwdbwd_ms"] = round(f[k], 4), round(fb[k], 4)
    rec["eval_fwd_torch_over_fused"] = round(f["torch"] / f["fused"], 2)
    rec["train_fwdbwd_torch_over_fused"] = round(fb["torch"] / fb["fused"], 2)
    return rec


def whole_model(dev, a):
    import time
    import statistics
    import ptv3_stand_in as S
    from gaussiancity_amd import point_attention, point_ffn, point_front, point_mid, point_pool, point_seam
    installs = (point_attention, point_pool, point_front, point_mid, point_ffn, point_seam)
    widths = tuple(int(w) for w in a.model_widths.split(","))
    torch.manual_seed(0)
    model = S.PointTransformerV3(cin=6, widths=widths, orders=("z", "z-trans")[:a.model_orders], patch_size=a.model_patch,
                                 depth=a.model_depth).to(dev).train()
    frame = {k: v.to(dev) for k, v in S.sloped_frame(a.model_points, a.model_batches, a.model_depth).items()}
    dout = torch.randn(a.model_points, widths[1] if len(widths) > 1 else widths[0], device=dev)

    wide = a.ffn_max_channels or None   # a third side: point_ffn.install(..., max_channels=wide), the rest as they are
    sides = ("none", "installed") + (("installed_ffn_wide",) if wide else ())

    def bind(side):
        for m in reversed(installs):
            m.uninstall(S.NAMESPACE)
        if side == "none":
            return
        for m in installs:
            if m is point_ffn and side == "installed_ffn_wide":
                m.install(S.NAMESPACE, max_channels=wide)
            else:
                m.install(S.NAMESPACE)

    def one_pass():
        model.zero_grad(set_to_none=True)
        data = dict(frame)
        data["feat"] = frame["feat"].clone().requires_grad_(True)
        out = model(data)
        (out.feat * dout).sum().backward()
        return out.feat.detach(), data["feat"].grad

    res, stats = {}, {}
    try:
        for side in sides:
            bind(side)
            for m in (point_front, point_mid, point_ffn, point_pool, point_seam):
                m.reset_stats()
            res[side] = one_pass()
            stats[side] = {m.__name__.split(".")[-1]: m.stats() for m in (point_front, point_mid, point_ffn, point_pool, point_seam)}
            stats[side]["point_ffn_split"] = point_ffn.split_stats()
        diff = {side: [float((g - w).abs().max() / w.abs().max()) for g, w in zip(res[side], res["none"])] for side in sides[1:]}
        times = {side: [] for side in sides}
        for _ in range(a.reps):
            for side in sides:
                bind(side)
                one_pass()  # the side's allocator and autotune state before its block
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.model_iters):
                    one_pass()
                torch.cuda.synchronize()
                times[side].append(1e3 * (time.perf_counter() - t0) / a.model_iters)
    finally:
        bind("none")
    none, fused = statistics.median(times["none"]), statistics.median(times["installed"])
    rec = {"shape": "whole PTv3 forward + backward (tools/ptv3_stand_in.py), six installs against none", "points": a.model_points,
           "batches": a.model_batches, "depth": a.model_depth, "widths": list(widths), "orders": a.model_orders,
           "patch": a.model_patch, "timing": "host wall ms per pass, blocks of %d ending in a synchronise, median of %d rounds"
           % (a.model_iters, a.reps), "none_ms": round(none, 3), "installed_ms": round(fused, 3),
           "none_over_installed": round(none / fused, 2), "none_ms_rounds": [round(t, 3) for t in times["none"]],
           "installed_ms_rounds": [round(t, 3) for t in times["installed"]],
           "installed_vs_none_max_rel_diff": {"output": diff["installed"][0], "input_gradient": diff["installed"][1]},
           "paths_taken_last_pass": {k: v for k, v in stats["installed"].items() if k != "point_ffn_split"}}
    if wide:
        w = statistics.median(times["installed_ffn_wide"])
        rec.update({"ffn_max_channels": wide, "installed_ffn_wide_ms": round(w, 3), "installed_over_installed_ffn_wide": round(fused / w, 3),
                    "none_over_installed_ffn_wide": round(none / w, 2),
                    "installed_ffn_wide_ms_rounds": [round(t, 3) for t in times["installed_ffn_wide"]],
                    "installed_ffn_wide_vs_none_max_rel_diff": {"output": diff["installed_ffn_wide"][0],
                                                                "input_gradient": diff["installed_ffn_wide"][1]},
                    "paths_taken_ffn_wide": stats["installed_ffn_wide"]})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=30, help="untimed calls of every side before its timed blocks")
    ap.add_argument("--out", default=None)
    ap.add_argument("--model-points", type=int, default=150000)
    ap.add_argument("--model-batches", type=int, default=57)
    ap.add_argument("--model-depth", type=int, default=8)
    ap.add_argument("--model-widths", default="32,64,128,256,512", help="config.py's encoder widths")
    ap.add_argument("--model-orders", type=int, default=1, help="serialization orders (GaussianCity: 1, `cord`)")
    ap.add_argument("--model-patch", type=int, default=1024)
    ap.add_argument("--model-iters", type=int, default=3)
    ap.add_argument("--ffn-max-channels", type=int, default=0,
                    help="a third side of the whole model: point_ffn.install(..., max_channels=this), the split feed-forward")
    ap.add_argument("--model-only", action="store_true", help="skip the seam shapes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seam_bench needs a GPU")
    dev = torch.device("cuda:0")
    bench_shape(dev, *SHAPES[0][:4], 100, 3, 50, "process warm-up, not reported")  # clocks up first
    lines = []
    for rows, I, O, product, label in ([] if a.model_only else SHAPES):
        rec = bench_shape(dev, rows, I, O, product, a.warmup, a.reps, a.iters, label)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    lines.append(whole_model(dev, a))
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
