"""Timing of the HIP submanifold convolution (gaussiancity_amd.sparse) on PTv3's distinct convolution shapes, against
a yardstick of torch ops on the same neighbour map (per tap: index_select + mm + index_add_, torch's own BLAS).

  python tools/sparse_bench.py [--reps 7] [--iters 10] [--inference-n 262144] [--out FILE] [--engine valu|mfma|both]
                               [--dtype float32|float16|both]

Clouds: a 16 384-point building shell (tests/sparse_ref.shell_cloud) pooled stage by stage (coords >> 1) gives the
N of every stage; the stage-0 shapes also run on an inference-sized shell of --inference-n points.  One JSON line per
shape: rulebook build, forward and forward + backward in ms (median over --reps blocks of --iters calls, device
events), the backward split (a backward asked for dX only and one asked for dW only, through the C ABI on buffers
allocated once, so that the figure is the device work and not the autograd layer around it), the present pairs, the FLOP and byte
floors of those pairs, the yardstick's forward and forward + backward, the dW slices of the plan and the products the
engine runs on the matrix cores.  --engine picks the engine of the convolution's three products
(gaussiancity_amd.sparse.set_engine); `both` runs the two engines one after the other shape by shape in this one
process and writes one line per shape and engine to profiles/sparse_bench_engines.jsonl (or --out): VALU against MFMA
is compared within that one process.  Every timing comes with the spread of its block medians
((max - min) / median over the --reps blocks).  --dtype float32, the default, is all of the above unchanged; float16 times
a .half() layer (the `_t` entry points, one engine, the f16 matrix cores; the yardstick then runs torch's float16 mm);
`both` alternates the float32 matrix-core engine and float16 shape by shape in this one process and writes to
profiles/sparse_bench_half.jsonl (or --out).  With --dtype float16 or both every line also carries `dtype` and
`worst_units`, the worst |y - float64| / unit over the forward's elements, unit = 2^-11 * sum |terms| + 2^-24 (the bar of
tests/test_sparse_half_gpu.py; the float32 lines are measured in the same unit).  Needs a GPU; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import sparse_ref as R  # noqa: E402
from gaussiancity_amd import sparse as SP  # noqa: E402


class Timing(float):
    """Median ms per call; `.spread` is (max - min) / median of the blocks it is the median of."""
    spread = 0.0


def timed(fn, reps, iters):
    """Median ms per call over `reps` blocks of `iters` calls, device events around each block."""
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
    t = Timing(statistics.median(out))
    t.spread = (max(out) - min(out)) / t if t > 0 else 0.0
    return t


def yardstick(x, w, bias, taps, dy):
    """Forward and forward + backward closures of the torch-ops version on the same neighbour map."""
    cout, K, cin = w.shape[0], taps["K"], x.shape[1]
    W = w.reshape(cout, K, cin)
    Wt = [W[:, k, :].t().contiguous() for k in range(K)]
    Wk = [W[:, k, :].contiguous() for k in range(K)]
    present = [k for k in range(K) if len(taps["rows"][k])]

    def fwd():
        y = bias.expand(x.shape[0], cout).clone() if bias is not None else x.new_zeros((x.shape[0], cout))
        for k in present:
            y.index_add_(0, taps["rows"][k], torch.mm(x.index_select(0, taps["cols"][k]), Wt[k]))
        return y

    def fwdbwd():
        fwd()
        dx = torch.zeros_like(x)
        dw = torch.zeros_like(W)
        for k in present:
            g = dy.index_select(0, taps["rows"][k])
            dx.index_add_(0, taps["cols"][k], torch.mm(g, Wk[k]))
            dw[:, k, :] = torch.mm(g.t(), x.index_select(0, taps["cols"][k]))
        return dx, dw, dy.sum(0)

    return fwd, fwdbwd


def bench_shape(dev, coords, cin, cout, k, bias, reps, iters, label, engine="valu", dtype=None):
    """`dtype` None: float32 and today's record; "float32" / "float16": that dtype, and the record gains `dtype` and
    `worst_units` (a float16 layer has one engine: `engine` is then only what the record's plan is read from, "mfma")."""
    import spconv.pytorch as spconv
    previous = SP.set_engine(engine)
    try:
        return _bench_shape(spconv, dev, coords, cin, cout, k, bias, reps, iters, label, engine, dtype)
    finally:
        SP.set_engine(previous)


def _bench_shape(spconv, dev, coords, cin, cout, k, bias, reps, iters, label, engine, dtype):
    half = dtype == "float16"
    n = len(coords)
    idx = torch.from_numpy(R.with_batch(coords, np.zeros(n))).to(dev)
    shape = (coords.max(0) + 3).tolist()
    g = torch.Generator(device="cpu").manual_seed(cin * 7 + k)
    x = torch.randn(n, cin, generator=g).to(dev)
    dy = torch.randn(n, cout, generator=g).to(dev)
    conv = spconv.SubMConv3d(cin, cout, k, bias=bias).to(dev)
    if half:
        x, dy, conv = x.half(), dy.half(), conv.half()
        for t in (x, dy, conv.weight.data) + ((conv.bias.data,) if bias else ()):
            t[t.abs() < 2.0 ** -14] = 0  # no binary16 subnormals (DESIGN.md section 15 says what the matrix cores do with them)
    t = spconv.SparseConvTensor(x, idx, shape, 1)

    builds = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rb = SP.Rulebook(idx, shape, 1, conv.kernel_size, conv.dilation)
        torch.cuda.synchronize()
        builds.append((time.perf_counter() - t0) * 1e3)
    pairs = sum(rb.pairs)
    xg = x.clone().requires_grad_(True)

    def fwd():
        with torch.no_grad():
            return SP.SubMConvFunction.apply(x, conv.weight, conv.bias, rb)

    def fwdbwd():
        y = SP.SubMConvFunction.apply(xg, conv.weight, conv.bias, rb)
        xg.grad = None
        conv.weight.grad = None
        if conv.bias is not None:
            conv.bias.grad = None
        y.backward(dy)

    fwd_ms, fb_ms = timed(fwd, reps, iters), timed(fwdbwd, reps, iters)

    def backward_only(want_x, want_w):
        """A backward asked for one gradient, through the C ABI on buffers allocated once: the device work, without the
        autograd layer's allocations around it."""
        eng, K = (SP.S.DTYPE_F16 if half else SP.S.ENGINES[engine]), rb.kvol
        ws_bytes = (SP.S.subm_workspace_bytes_t(eng, n, cin, cout, K, rb.dups)[1] if half else
                    SP.S.subm_engine_workspace_bytes(eng, n, cin, cout, K, rb.dups)[1])
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        w = conv.weight.detach()
        dx = torch.empty_like(x) if want_x else None
        dw = torch.empty_like(w) if want_w else None
        args = (eng, rb.buf.data_ptr(), n, K, rb.dups, x.data_ptr(), cin, w.data_ptr(), cout, dy.data_ptr(),
                dx.data_ptr() if want_x else None, dw.data_ptr() if want_w else None, None, ws.data_ptr(), ws_bytes,
                SP._stream())
        call = SP.S.lib().gcs_subm_backward_t if half else SP.S.lib().gcs_subm_backward_engine

        def run():
            SP.S.check(call(*args), "gcs_subm_backward_t" if half else "gcs_subm_backward_engine")

        run.buffers = (ws, dx, dw)  # the pointers in `args` stay valid as long as the closure lives
        return run

    dx_ms, dw_ms = timed(backward_only(True, False), reps, iters), timed(backward_only(False, True), reps, iters)

    nbr = R.neighbours(R.with_batch(coords, np.zeros(n)), shape, conv.kernel_size, conv.dilation)
    taps = {"K": nbr.shape[1], "rows": [], "cols": []}
    for q in range(nbr.shape[1]):
        rows = np.nonzero(nbr[:, q] >= 0)[0]
        taps["rows"].append(torch.from_numpy(rows).to(dev))
        taps["cols"].append(torch.from_numpy(nbr[rows, q]).to(dev))
    assert sum(len(r) for r in taps["rows"]) == pairs
    with torch.no_grad():
        yf, yb = yardstick(x, conv.weight.detach(), None if conv.bias is None else conv.bias.detach(), taps, dy)
        y_ref = yf()
        y_got = fwd()
        agree = float((y_got.float() - y_ref.float()).abs().max()) / max(1e-30, float(y_ref.float().abs().max()))
        tf_ms, tfb_ms = timed(yf, reps, iters), timed(yb, reps, iters)
    K = nbr.shape[1]
    flop_f = 2.0 * pairs * cin * cout
    bytes_f = (2.0 if half else 4.0) * (n * cin + n * cout + K * cin * cout) + 4.0 * n * K
    plan = SP.S.subm_engine_plan(SP.S.ENGINES[engine], n, cin, cout, K)
    extra = {}
    if dtype is not None:
        f64 = lambda t: None if t is None else t.detach().double().cpu().numpy()  # noqa: E731
        ry, sy = R.conv_forward(f64(x), f64(conv.weight), f64(conv.bias), nbr)
        units = np.abs(y_got.double().cpu().numpy() - ry) / (2.0 ** -11 * sy + 2.0 ** -24)
        extra = {"dtype": dtype, "worst_units": round(float(units.max()), 3)}
    return {**extra, "shape": label, "engine": "half" if half else engine, "engine_products": list(SP.engine_products(engine)),
            "fwd_slices": plan[5], "dx_slices": plan[6], "dw_slices": plan[3],
            "dx_ms": round(dx_ms, 4), "dx_spread": round(dx_ms.spread, 4),
            "dw_ms": round(dw_ms, 4), "dw_spread": round(dw_ms.spread, 4),
            "fwd_spread": round(fwd_ms.spread, 4), "fwdbwd_spread": round(fb_ms.spread, 4), "cin": cin, "cout": cout, "k": k, "n": n, "pairs": pairs,
            "rulebook_ms": round(statistics.median(builds), 4), "fwd_ms": round(fwd_ms, 4), "fwdbwd_ms": round(fb_ms, 4),
            "torch_fwd_ms": round(tf_ms, 4), "torch_fwdbwd_ms": round(tfb_ms, 4),
            "fwd_speedup": round(tf_ms / fwd_ms, 2), "fwdbwd_speedup": round(tfb_ms / fb_ms, 2),
            "flop_fwd": flop_f, "flop_fwdbwd": 3 * flop_f, "bytes_floor_fwd": bytes_f,
            "fwd_tflops": round(flop_f / fwd_ms / 1e9, 3), "fwdbwd_tflops": round(3 * flop_f / fb_ms / 1e9, 3),
            "max_rel_diff_vs_yardstick": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--inference-n", type=int, default=262144)
    ap.add_argument("--out", default=None)
    ap.add_argument("--engine", choices=["valu", "mfma", "both"], default="valu")
    ap.add_argument("--dtype", choices=["float32", "float16", "both"], default="float32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_bench needs a GPU")
    dev = torch.device("cuda:0")
    stages = R.pool_stages(R.shell_cloud(16384, 2024), 4)
    cases = [(stages[st], cin, cout, k, k == 3, "%d->%d k%d stage%d" % (cin, cout, k, st)) for cin, cout, k, st in R.PTV3_SHAPES]
    if a.inference_n:
        big = R.shell_cloud(a.inference_n, 99, extent=640, size=(8, 96))
        cases += [(big, 128, 32, 5, False, "128->32 k5 inference"), (big, 32, 32, 3, True, "32->32 k3 inference")]
    lines = []
    for coords, cin, cout, k, bias, label in cases:
        if a.dtype == "float32":
            runs = [(engine, None) for engine in (("valu", "mfma") if a.engine == "both" else (a.engine,))]
        else:  # float16 has one engine; its float32 partner in `both` is the matrix-core engine
            runs = [("mfma", "float32"), ("mfma", "float16")] if a.dtype == "both" else [("mfma", "float16")]
        for engine, dtype in runs:
            rec = bench_shape(dev, coords, cin, cout, k, bias, a.reps, a.iters, label, engine, dtype)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    out = a.out or (os.path.join(ROOT, "profiles", "sparse_bench_half.jsonl") if a.dtype == "both" else
                    os.path.join(ROOT, "profiles", "sparse_bench_engines.jsonl") if a.engine == "both" else None)
    if out:
        with open(out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
