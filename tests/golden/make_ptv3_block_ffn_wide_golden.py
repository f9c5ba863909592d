#!/usr/bin/env python
"""Generates tests/golden/ptv3_block_ffn_wide.npz with the REFERENCE's own models/pt_v3.py, imported on the CPU, after
make_ptv3_block_ffn_golden.py (same imports, same arrays per case, data only): the last third of Block.forward (pre_norm)
at a width beyond the one-launch feed-forward kernels' 128 channels, for point_ffn.install(..., max_channels=512).  Run in
the build container only (the reference does not exist on the GPU box):

    python tests/golden/make_ptv3_block_ffn_wide_golden.py <reference root>

One case, c132: 65 rows, C = 132 -- the smallest width beyond the old cap -- and MLP(hidden_channels=72): two chunks of 64
hidden features of which the second is partial.  (A C = 256, hidden 1024 case runs through this generator unchanged apart
from the sizes, but its file is 6.4 MB: beyond what a committed fixture may be.)  Per case <c> the arrays are those of
ptv3_block_ffn.npz:

    <c>.feat, <c>.w, <c>.eps, <c>.norm.weight ... <c>.fc2.bias, <c>.out, <c>.grad.<tensor>, <c>.err32.<tensor>
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_ptv3_index_golden import ROOT, reference_module  # noqa: E402

CASES = {"c132": (65, 132, 72)}  # rows, channels, hidden channels
PARAMS = ("norm.weight", "norm.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


def run(M, dtype, C, Hd, feat, w, params):
    norm2 = M.PointSequential(torch.nn.LayerNorm(C)).to(dtype)
    mlp = M.PointSequential(M.MLP(in_channels=C, hidden_channels=Hd, out_channels=C, act_layer=torch.nn.GELU)).to(dtype)
    drop_path = M.PointSequential(torch.nn.Identity())
    own = {"norm.weight": norm2[0].weight, "norm.bias": norm2[0].bias, "fc1.weight": mlp[0].fc1.weight,
           "fc1.bias": mlp[0].fc1.bias, "fc2.weight": mlp[0].fc2.weight, "fc2.bias": mlp[0].fc2.bias}
    with torch.no_grad():
        for name, value in params.items():
            own[name].copy_(torch.from_numpy(value).to(dtype))
    x = torch.from_numpy(feat).to(dtype).requires_grad_(True)
    point = M.Point(feat=x)
    shortcut = point.feat                      # Block.forward from `shortcut = point.feat` on, pre_norm
    point = norm2(point)
    point = drop_path(mlp(point))
    point.feat = shortcut + point.feat
    out = point.feat
    (out * torch.from_numpy(w).to(dtype)).sum().backward()
    res = {"out": out.detach().numpy(), "grad.feat": x.grad.numpy()}
    res.update({"grad." + name: own[name].grad.numpy() for name in PARAMS})
    return res, float(norm2[0].eps)


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "models", "pt_v3.py")):
        raise SystemExit("usage: make_ptv3_block_ffn_wide_golden.py <reference root> (the directory that holds models/pt_v3.py)")
    M = reference_module(sys.argv[1])
    rng = np.random.default_rng(20261021)
    blob = {}
    for case, (n, C, Hd) in CASES.items():
        feat = rng.normal(size=(n, C)).astype(np.float32)
        w = rng.normal(size=(n, C)).astype(np.float32)
        params = {"norm.weight": 1.0 + 0.5 * rng.normal(size=C), "norm.bias": 0.1 * rng.normal(size=C),
                  "fc1.weight": rng.normal(size=(Hd, C)) * C ** -0.5, "fc1.bias": 0.1 * rng.normal(size=Hd),
                  "fc2.weight": rng.normal(size=(C, Hd)) * Hd ** -0.5, "fc2.bias": 0.1 * rng.normal(size=C)}
        params = {k: v.astype(np.float32) for k, v in params.items()}
        r64, eps = run(M, torch.float64, C, Hd, feat, w, params)
        r32, _ = run(M, torch.float32, C, Hd, feat, w, params)
        blob.update({"%s.feat" % case: feat, "%s.w" % case: w, "%s.eps" % case: np.asarray(eps)})
        blob.update({"%s.%s" % (case, k): v for k, v in params.items()})
        for name, x64 in r64.items():
            assert x64.dtype == np.float64 and r32[name].dtype == np.float32
            blob["%s.%s" % (case, name)] = x64
            err = float(np.abs(r32[name].astype(np.float64) - x64).max() / np.abs(x64).max())
            blob["%s.err32.%s" % (case, name)] = np.asarray(err)
            print(case, name, "float32 run: %.2e of the maximum" % err)
    path = os.path.join(ROOT, "tests", "golden", "ptv3_block_ffn_wide.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes,", len(blob), "arrays")


if __name__ == "__main__":
    main()
