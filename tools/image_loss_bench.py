"""The image losses (include/gcv.h K20-K22, gaussiancity_amd/image_loss.py) against upstream's own torch lines on the
device -- image_loss.torch_l1 / torch_gan_loss / torch_label_map, which are core/train.py:285, losses/gan.py:55-97 and
models/discriminator.py:177-189 as torch runs them -- at the shapes of a training step:

  l1         (1,3,448,448) and (1,3,448,224) with a mask, (1,256,112,112) without
  gan_loss   both modes at (1,9,112,112) and (1,9,112,56) with weights
  label_map  448 x 448 -> 112 x 112, 8 classes, with the mask

Both sides run in one process on the same stream, alternating, around blocks of calls that end in a synchronise; host
wall time per call, median over the blocks; forward alone (under no_grad) and forward + backward.  Launches per call are
counted with torch.profiler in a pass of their own after the timing.  The results are compared on every case.  Appends one
JSON line to --out.
    python tools/image_loss_bench.py --out profiles/image_loss.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussiancity_amd import image_loss as IL  # noqa: E402


def count_launches(fn):
    """Device kernels and memcpys one call of fn enqueues, or None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev_type = getattr(torch.autograd.DeviceType, "CUDA")
        return sum(1 for e in prof.events() if e.device_type == dev_type) or None
    except Exception as e:  # noqa: BLE001 -- a count is informational; the timing stands without it
        print("launch count not available: %r" % (e,), file=sys.stderr)
        return None


def ab(sides, calls, blocks):
    """{name: median ms per call}, and the per-block values; the sides alternate block by block."""
    for fn in sides.values():
        for _ in range(2):
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
    wall = {name: [] for name in sides}
    for _ in range(blocks):
        for name, fn in sides.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            wall[name].append(1e3 * (time.perf_counter() - t0) / calls)
    return {name: round(statistics.median(v), 5) for name, v in wall.items()}, {name: [round(x, 5) for x in v] for name, v in wall.items()}


def make_cases(dev):
    gen = torch.Generator().manual_seed(11)

    def rnd(*shape):
        return (torch.rand(shape, generator=gen) * 2.4 - 1.2).to(dev)

    cases = []
    for shape, masked in (((1, 3, 448, 448), True), ((1, 3, 448, 224), True), ((1, 256, 112, 112), False)):
        a, b = rnd(*shape).requires_grad_(True), rnd(*shape)
        m = (torch.rand((shape[0], 1) + shape[2:], generator=gen) < 0.7).float().to(dev) if masked else None
        cases.append(("l1 %s%s" % ("x".join(map(str, shape)), " masked" if masked else ""), a,
                      lambda a=a, b=b, m=m: IL.l1(a, b, m), lambda a=a, b=b, m=m: IL.torch_l1(a, b, m)))
    for shape in ((1, 9, 112, 112), (1, 9, 112, 56)):
        B, C1, h, w = shape
        pred = (torch.randn(shape, generator=gen) * 3).to(dev).requires_grad_(True)
        cls = torch.randint(0, C1 - 1, (B, 1, h, w), generator=gen)
        label = torch.zeros((B, C1 - 1, h, w)).scatter_(1, cls, 1.0).to(dev)
        weight = (torch.rand((B, 1, h, w), generator=gen) < 0.7).float().to(dev)
        for real in (True, False):
            cases.append(("gan_loss %s %s" % ("x".join(map(str, shape)), "real" if real else "fake"), pred,
                          lambda p=pred, l=label, wt=weight, r=real: IL.gan_loss(p, l, wt, real=r),
                          lambda p=pred, l=label, wt=weight, r=real: IL.torch_gan_loss(p, l, wt, r)))
    cls = torch.randint(0, 8, (1, 1, 448, 448), generator=gen)
    seg = torch.zeros((1, 8, 448, 448)).scatter_(1, cls, 1.0).to(dev)
    mask = (torch.rand((1, 1, 448, 448), generator=gen) < 0.7).float().to(dev)
    cases.append(("label_map 448x448->112x112 C=8 masked", None,
                  lambda: IL.label_map(seg, (112, 112), mask), lambda: IL.torch_label_map(seg, (112, 112), mask)))
    return cases


def with_backward(fn, leaf):
    def run():
        leaf.grad = None
        fn().backward()
    return run


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="calls per timed block")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_loss.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_loss_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    IL.reset_stats()
    rows, ok = [], True
    for name, leaf, device_fn, torch_fn in make_cases(dev):
        rec = {"case": name}
        d, t = device_fn(), torch_fn()
        if leaf is None:
            rec["check"] = {"bit_for_bit": bool(torch.equal(d, t))}
            ok = ok and rec["check"]["bit_for_bit"]
        else:
            leaf.grad = None
            d.backward()
            gd, leaf.grad = leaf.grad, None
            t.backward()
            gt, leaf.grad = leaf.grad, None
            rel = abs(d.item() - t.item()) / max(abs(t.item()), 1e-30)
            gerr = float((gd - gt).abs().max()) / max(float(gt.abs().max()), 1e-30)
            rec["check"] = {"loss_relative_difference": rel, "gradient_difference_over_max": gerr}
            ok = ok and rel <= 1e-5 and gerr <= 1e-5
        fwd, fwd_blocks = ab({"torch": no_grad(torch_fn), "device": no_grad(device_fn)}, args.calls, args.blocks)
        rec["forward"] = {"ms_per_call": fwd, "torch_over_device": round(fwd["torch"] / fwd["device"], 2), "ms_blocks": fwd_blocks,
                          "launches": {"torch": count_launches(no_grad(torch_fn)), "device": count_launches(no_grad(device_fn))}}
        if leaf is not None:
            sides = {"torch": with_backward(torch_fn, leaf), "device": with_backward(device_fn, leaf)}
            both, both_blocks = ab(sides, args.calls, args.blocks)
            rec["forward_backward"] = {"ms_per_call": both, "torch_over_device": round(both["torch"] / both["device"], 2),
                                       "ms_blocks": both_blocks,
                                       "launches": {k: count_launches(fn) for k, fn in sides.items()}}
        rows.append(rec)
        print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "ms_blocks"} if isinstance(v, dict) else v) for k, v in rec.items()}), flush=True)
    rec = {"tool": "tools/image_loss_bench.py", "device": torch.cuda.get_device_name(0),
           "timing": "host wall time per call around blocks of %d calls ending in a synchronise; both sides in one process on one "
                     "stream, alternating; median of %d blocks; forward under no_grad, forward + backward with the gradient of "
                     "the first input" % (args.calls, args.blocks),
           "yardstick": "image_loss.torch_l1 / torch_gan_loss / torch_label_map: upstream's torch lines on the device",
           "cases": rows, "stats": IL.stats()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    if not ok:
        raise SystemExit("device and torch results differ")


if __name__ == "__main__":
    main()
