"""Timing of the attribute head's output layers in a training step (gaussiancity_amd.modlinear.head_attrs / head_points14,
DESIGN.md section 17c) against the torch lines they replace, on the same inputs in one process.

  python tools/head_train_bench.py [--reps 7] [--iters 10] [--warmup 30] [--out profiles/head_train.jsonl]

Shape: N = 16 384 rows, I = 512 hidden features.  Keys: {"rgb"} alone (the config default) and all four.  Variants: with and
without a group vector (about 5 % of the rows at -1); the dict form and the [N, 14] form.
Sides: `hip`, the operator; `torch`, per key fc_out (F.linear), the sigmoid / clamp transform and torch.where over the
covered rows (attr_head's tail with gradients), and for the [N, 14] form helpers.get_gaussian_points on clones of xyz and
scales -- both sides on the device, from the same hidden activations (one h per key, as the head's per-key layers leave
them).  Protocol of tools/front_bench.py: --warmup untimed calls of each side, then --reps rounds in which each side runs one
block of --iters calls between device events; the median block per side.  One JSON line per variant: forward + backward in
ms per side, the forward alone with gradients enabled (so `pre` is stored), the ratio torch / hip (above 1 the operator is
faster; whatever comes out is written down), the launches of the hip side, and peak allocator bytes of one forward +
backward per side.  Needs a GPU; there is no CPU path."""
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
from gaussiancity_amd import helpers, modlinear  # noqa: E402

N, I = 16384, 512
FACTORS = {"xyz": 0.75, "rgb": 2.0, "scale": 0.5, "opacity": 0.6}
KEY_SETS = {"rgb": ("rgb",), "four": ("xyz", "rgb", "scale", "opacity")}


def torch_attrs(keys, group):
    covered = None if group is None else (group >= 0).unsqueeze(1)
    out = {}
    for k, (h, w, b, factor) in keys.items():
        v = F.linear(h, w, b)
        if k == "scale":
            v = 1 + v.clamp(-1, 1) * factor
        elif k == "opacity":
            v = torch.sigmoid(v) * factor + (1 - factor)
        else:
            v = (torch.sigmoid(v) - 0.5) * factor
        out[k] = v if covered is None else torch.where(covered, v, torch.zeros((), dtype=v.dtype, device=v.device))
    return out


def make(dev, kinds, seed):
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    keys = {}
    for k in kinds:
        C = 1 if k == "opacity" else 3
        keys[k] = (n(N, I).to(dev).requires_grad_(True), (n(C, I) / I ** 0.5 * (3.0 if k == "scale" else 1.0)).to(dev).requires_grad_(True),
                   (0.3 * n(C)).to(dev).requires_grad_(True), FACTORS[k])
    group = torch.randint(0, 8, (N,), generator=g, dtype=torch.int32)
    group[torch.rand(N, generator=g) < 0.05] = -1
    douts = [n(N, 1 if k == "opacity" else 3).to(dev) for k in kinds]
    return keys, group.to(dev), n(N, 3).to(dev), (0.5 + torch.rand(N, 3, generator=g)).to(dev), douts, n(N, 14).to(dev)


def bench_variant(dev, name, kinds, grouped, packed, warmup, reps, iters):
    keys, group, xyz, scales, douts, dp = make(dev, kinds, len(kinds) + 2 * grouped + packed)
    group = group if grouped else None
    leaves = [t for h, w, b, _ in keys.values() for t in (h, w, b)]

    def forward(side):
        if side == "hip":
            return modlinear.head_points14(keys, xyz, scales, group) if packed else modlinear.head_attrs(keys, group)
        attrs = torch_attrs(keys, group)
        if not packed:
            return attrs
        return helpers.get_gaussian_points(xyz.clone().unsqueeze(0), scales.clone().unsqueeze(0),
                                           {k: v.unsqueeze(0) for k, v in attrs.items()})[0]

    def fwd(side):
        return lambda: forward(side)

    def fwdbwd(side):
        def run():
            for t in leaves:
                t.grad = None
            out = forward(side)
            if packed:
                out.backward(dp)
            else:
                torch.autograd.backward(list(out.values()), douts)
        return run

    rec = {"variant": name, "rows": N, "hidden": I, "keys": list(kinds), "group": grouped, "form": "points14" if packed else "dict",
           "hip_launches_fwd": 1, "hip_launches_bwd": 2}
    with torch.no_grad():   # the two sides compute the same thing
        a, b = forward("hip"), forward("torch")
        pairs = [(a, b)] if packed else [(a[k], b[k]) for k in kinds]
        rec["max_abs_diff_fwd"] = max(float((x - y).abs().max()) for x, y in pairs)
    f = timed_sides({k: fwd(k) for k in ("hip", "torch")}, warmup, reps, iters)
    fb = timed_sides({k: fwdbwd(k) for k in ("hip", "torch")}, warmup, reps, iters)
    for k in ("hip", "torch"):
        rec[k + "_fwd_ms"], rec[k + "_fwdbwd_ms"] = round(f[k], 4), round(fb[k], 4)
        rec[k + "_peak_bytes"] = peak_bytes(fwdbwd(k), leaves)
    rec["fwd_torch_over_hip"] = round(f["torch"] / f["hip"], 2)
    rec["fwdbwd_torch_over_hip"] = round(fb["torch"] / fb["hip"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=30, help="untimed calls of every side before its timed blocks")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_train_bench needs a GPU")
    dev = torch.device("cuda:0")
    bench_variant(dev, "process warm-up, not reported", KEY_SETS["four"], True, True, 100, 3, 50)  # clocks up before the first variant
    lines = []
    for kname, kinds in KEY_SETS.items():
        for grouped in (False, True):
            for packed in (False, True):
                name = "%s keys, %s, %s" % (kname, "group" if grouped else "no group", "points14" if packed else "dict")
                rec = bench_variant(dev, name, kinds, grouped, packed, a.warmup, a.reps, a.iters)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
