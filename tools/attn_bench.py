"""Timing of the HIP variable-length attention (the flash_attn drop-in, gaussiancity_amd.attention) on PTv3's
SerializedAttention shapes, against two yardsticks of plain torch on the same inputs.

  python tools/attn_bench.py [--reps 7] [--iters 10] [--warmup 30] [--inference-n 262144] [--out FILE]

Shapes: the five encoder stages of a 16 384-point shell (16 384 / 4 292 / 1 063 / 271 / 73 rows, padded as PTv3 pads
them: to whole patches of 1024 when longer than one patch, else one short segment; 2 / 4 / 8 / 16 / 32 heads of 16
channels) and stage 0 of an inference-sized shell.  Yardsticks:
  torch_fp32   the backbone's non-flash formulation: fp32 [patches, H, K, d], (q * scale) @ k^T, softmax, @ v, with
               the [patches, H, K, K] scores kept for the backward (only where every segment is a whole patch);
  sdpa_fp16    torch.nn.functional.scaled_dot_product_attention on the same float16 values.
One JSON line per shape: forward and forward + backward in ms (median over --reps blocks of --iters calls, device
events, after --warmup untimed calls), the largest difference from the same formula in float64, peak allocator bytes of one forward + backward of each, the FLOP count 4 * sum(len^2) * H * d (forward;
3.5 x that for forward + backward) and the achieved TFLOP/s.  Needs a GPU; there is no CPU path.

  python tools/attn_bench.py --dtype float32 [--out profiles/attn_bench_f32.jsonl]

times the float32 kernels (attention.varlen_attention on float32 inputs) on the same shapes with the same protocol.
Yardsticks: torch_fp32 as above on the same float32 values, and kernels_fp16, the binary16 kernels on the values rounded
to float16.  The difference from float64 is reported for the float32 kernels and for torch_fp32."""
import argparse
import itertools
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import flash_attn  # noqa: E402

PATCH, D = 1024, 16
STAGES = [(16384, 2), (4292, 4), (1063, 8), (271, 16), (73, 32)]


WARMUP = 30


def timed(fn, reps, iters):
    """Median ms per call over `reps` blocks of `iters` calls, device events around each block, after WARMUP
    untimed calls (code objects loaded, allocator blocks cached, clocks up)."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out)


def peak_bytes(fn, leaf):
    """Allocator bytes above the resident inputs while one call of fn runs (the leaf's previous gradient dropped first)."""
    leaf.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def padded(rows):
    return -(-rows // PATCH) * PATCH if rows > PATCH else rows


def bench_shape(dev, rows, heads, reps, iters, label):
    total = padded(rows)
    whole = total % PATCH == 0
    lens = [PATCH] * (total // PATCH) if whole else [total]
    scale = D ** -0.5
    g = torch.Generator(device="cpu").manual_seed(rows + heads)
    qkv = torch.randn(total, 3, heads, D, generator=g).half().to(dev)
    dout = torch.randn(total, heads, D, generator=g).half().to(dev)
    cu = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32, device=dev)
    xg = qkv.clone().requires_grad_(True)

    def fwd():
        with torch.no_grad():
            return flash_attn.flash_attn_varlen_qkvpacked_func(qkv, cu, PATCH, softmax_scale=scale)

    def fwdbwd():
        xg.grad = None
        flash_attn.flash_attn_varlen_qkvpacked_func(xg, cu, PATCH, softmax_scale=scale).backward(dout)

    # [segments, H, len, d] views of the same values for the yardsticks
    def split(x):
        return x.reshape(len(lens), lens[0], 3, heads, D).permute(2, 0, 3, 1, 4)

    x16 = qkv.clone().requires_grad_(True)
    x32 = qkv.float().requires_grad_(True)
    dy = dout.reshape(len(lens), lens[0], heads, D).permute(0, 2, 1, 3)

    def sdpa(train):
        def run():
            x16.grad = None
            with torch.set_grad_enabled(train):
                q, k, v = split(x16)
                o = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=scale)
                if train:
                    o.backward(dy)
            return o
        return run

    def fp32(train):
        def run():
            x32.grad = None
            with torch.set_grad_enabled(train):
                q, k, v = split(x32)
                o = torch.softmax((q * scale) @ k.transpose(-2, -1), dim=-1) @ v
                if train:
                    o.backward(dy.float())
            return o
        return run

    # agreement with the same formula in float64, a few segments at a time
    got, agree = fwd().reshape(len(lens), lens[0], heads, D), 0.0
    with torch.no_grad():
        q, k, v = split(qkv)
        for s0 in range(0, len(lens), 16):
            qq, kk, vv = (t[s0:s0 + 16].double() for t in (q, k, v))
            want = torch.softmax(scale * (qq @ kk.transpose(-2, -1)), dim=-1) @ vv
            agree = max(agree, float((got[s0:s0 + 16].double() - want.permute(0, 2, 1, 3)).abs().max()))
    flop = 4.0 * sum(n * n for n in lens) * heads * D
    rec = {"shape": label, "rows": rows, "padded_rows": total, "heads": heads, "head_dim": D, "segments": len(lens),
           "flop_fwd": flop, "flop_fwdbwd": 3.5 * flop, "qkv_bytes": qkv.numel() * 2,
           "max_abs_diff_vs_float64": agree}
    rec["fwd_ms"], rec["fwdbwd_ms"] = round(timed(fwd, reps, iters), 4), round(timed(fwdbwd, reps, iters), 4)
    rec["fwd_tflops"] = round(flop / rec["fwd_ms"] / 1e9, 3)
    rec["fwdbwd_tflops"] = round(3.5 * flop / rec["fwdbwd_ms"] / 1e9, 3)
    rec["peak_bytes"] = peak_bytes(fwdbwd, xg)
    rec["sdpa_fp16_fwd_ms"], rec["sdpa_fp16_fwdbwd_ms"] = round(timed(sdpa(False), reps, iters), 4), round(timed(sdpa(True), reps, iters), 4)
    rec["sdpa_fp16_peak_bytes"] = peak_bytes(sdpa(True), x16)
    rec["fwd_speedup_vs_sdpa_fp16"] = round(rec["sdpa_fp16_fwd_ms"] / rec["fwd_ms"], 2)
    rec["fwdbwd_speedup_vs_sdpa_fp16"] = round(rec["sdpa_fp16_fwdbwd_ms"] / rec["fwdbwd_ms"], 2)
    if whole:
        rec["torch_fp32_fwd_ms"], rec["torch_fp32_fwdbwd_ms"] = round(timed(fp32(False), reps, iters), 4), round(timed(fp32(True), reps, iters), 4)
        rec["torch_fp32_peak_bytes"] = peak_bytes(fp32(True), x32)
        rec["fwd_speedup_vs_torch_fp32"] = round(rec["torch_fp32_fwd_ms"] / rec["fwd_ms"], 2)
        rec["fwdbwd_speedup_vs_torch_fp32"] = round(rec["torch_fp32_fwdbwd_ms"] / rec["fwdbwd_ms"], 2)
    return rec


def bench_shape32(dev, rows, heads, reps, iters, label):
    """bench_shape for the float32 kernels: the same shape, inputs of the same seed kept in float32."""
    from gaussiancity_amd.attention import varlen_attention
    total = padded(rows)
    whole = total % PATCH == 0
    lens = [PATCH] * (total // PATCH) if whole else [total]
    scale = D ** -0.5
    g = torch.Generator(device="cpu").manual_seed(rows + heads)
    qkv = torch.randn(total, 3, heads, D, generator=g).to(dev)
    dout = torch.randn(total, heads, D, generator=g).to(dev)
    cu = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32, device=dev)
    leaves = {"f32": qkv.clone().requires_grad_(True), "f16": qkv.half().requires_grad_(True),
              "torch": qkv.clone().requires_grad_(True)}
    d16 = dout.half()
    dy = dout.reshape(len(lens), lens[0], heads, D).permute(0, 2, 1, 3)

    def kernels(which, train):
        x, gy = leaves[which], (dout if which == "f32" else d16)

        def run():
            x.grad = None
            with torch.set_grad_enabled(train):
                o = varlen_attention(x, cu, PATCH, softmax_scale=scale)
                if train:
                    o.backward(gy)
            return o
        return run

    def split(x):
        return x.reshape(len(lens), lens[0], 3, heads, D).permute(2, 0, 3, 1, 4)

    def fp32(train):
        x = leaves["torch"]

        def run():
            x.grad = None
            with torch.set_grad_enabled(train):
                q, k, v = split(x)
                o = torch.softmax((q * scale) @ k.transpose(-2, -1), dim=-1) @ v
                if train:
                    o.backward(dy)
            return o
        return run

    got = kernels("f32", False)().reshape(len(lens), lens[0], heads, D)
    agree = agree_torch = 0.0
    with torch.no_grad():
        q, k, v = split(qkv)
        for s0 in range(0, len(lens), 16):
            qq, kk, vv = (t[s0:s0 + 16].double() for t in (q, k, v))
            want = (torch.softmax(scale * (qq @ kk.transpose(-2, -1)), dim=-1) @ vv).permute(0, 2, 1, 3)
            agree = max(agree, float((got[s0:s0 + 16].double() - want).abs().max()))
            if whole:
                qf, kf, vf = (t[s0:s0 + 16] for t in (q, k, v))
                o32 = (torch.softmax((qf * scale) @ kf.transpose(-2, -1), dim=-1) @ vf).permute(0, 2, 1, 3)
                agree_torch = max(agree_torch, float((o32.double() - want).abs().max()))
    flop = 4.0 * sum(n * n for n in lens) * heads * D
    rec = {"shape": label, "dtype": "float32", "rows": rows, "padded_rows": total, "heads": heads, "head_dim": D,
           "segments": len(lens), "flop_fwd": flop, "flop_fwdbwd": 3.5 * flop, "qkv_bytes": qkv.numel() * 4,
           "max_abs_diff_vs_float64": agree}
    rec["fwd_ms"] = round(timed(kernels("f32", False), reps, iters), 4)
    rec["fwdbwd_ms"] = round(timed(kernels("f32", True), reps, iters), 4)
    rec["fwd_tflops"] = round(flop / rec["fwd_ms"] / 1e9, 3)
    rec["fwdbwd_tflops"] = round(3.5 * flop / rec["fwdbwd_ms"] / 1e9, 3)
    rec["peak_bytes"] = peak_bytes(kernels("f32", True), leaves["f32"])
    rec["kernels_fp16_fwd_ms"] = round(timed(kernels("f16", False), reps, iters), 4)
    rec["kernels_fp16_fwdbwd_ms"] = round(timed(kernels("f16", True), reps, iters), 4)
    rec["kernels_fp16_peak_bytes"] = peak_bytes(kernels("f16", True), leaves["f16"])
    rec["fwd_ratio_to_kernels_fp16"] = round(rec["fwd_ms"] / rec["kernels_fp16_fwd_ms"], 2)
    rec["fwdbwd_ratio_to_kernels_fp16"] = round(rec["fwdbwd_ms"] / rec["kernels_fp16_fwdbwd_ms"], 2)
    if whole:
        rec["torch_fp32_max_abs_diff_vs_float64"] = agree_torch
        rec["torch_fp32_fwd_ms"] = round(timed(fp32(False), reps, iters), 4)
        rec["torch_fp32_fwdbwd_ms"] = round(timed(fp32(True), reps, iters), 4)
        rec["torch_fp32_peak_bytes"] = peak_bytes(fp32(True), leaves["torch"])
        rec["fwd_speedup_vs_torch_fp32"] = round(rec["torch_fp32_fwd_ms"] / rec["fwd_ms"], 2)
        rec["fwdbwd_speedup_vs_torch_fp32"] = round(rec["torch_fp32_fwdbwd_ms"] / rec["fwdbwd_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=("float16", "float32"), default="float16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=30, help="untimed calls before the timed blocks of every closure")
    ap.add_argument("--inference-n", type=int, default=262144)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    globals()["WARMUP"] = a.warmup
    if not torch.cuda.is_available():
        raise SystemExit("attn_bench needs a GPU")
    dev = torch.device("cuda:0")
    cases = [(rows, heads, "stage%d %d rows H%d" % (i, rows, heads)) for i, (rows, heads) in enumerate(STAGES)]
    if a.inference_n:
        cases.append((a.inference_n, 2, "stage0 inference %d rows H2" % a.inference_n))
    bench = bench_shape32 if a.dtype == "float32" else bench_shape
    bench(dev, STAGES[0][0], STAGES[0][1], 3, 200, "process warm-up, not reported")  # clocks up before the first shape
    lines = []
    for rows, heads, label in cases:
        rec = bench(dev, rows, heads, a.reps, a.iters, label)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
