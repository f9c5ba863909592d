#!/usr/bin/env python
"""Generates tests/golden/ptv3_block_front.npz with the REFERENCE's own models/pt_v3.py, imported on the CPU: what
Block.forward (pre_norm) runs between its sparse convolution and its attention -- the rest of cpe, PointSequential(Linear(C,
C), LayerNorm(C)) on the convolution's output, the residual add, PointSequential(LayerNorm(C)) and SerializedAttention's
qkv projection, composed as the method and SerializedAttention.forward compose them -- run twice per case on the same seeded
parameters and inputs, once in float64 (the target) and once in float32 (the reference's own error).  Run in the build
container only (the reference does not exist on the GPU box):

    python tests/golden/make_ptv3_block_front_golden.py <reference root>

As make_ptv3_block_ffn_golden.py: the repository root goes first on sys.path, so that pt_v3.py's `spconv`, `flash_attn`
and `torch_scatter` are the drop-ins of this repository, and a dict with attribute access stands in for `addict`.  The
fixture holds inputs, parameters and the reference's outputs -- data only.  Per case <c>:

    <c>.feat, <c>.conv                       float32 [n, C]: the Block's input features (its shortcut) and the output of
                                             the sparse convolution, which the test's stand-in convolution returns
    <c>.w.feat, <c>.w.qkv                    float32 weights of the loss (feat * w.feat).sum() + (qkv * w.qkv).sum()
    <c>.eps.cpe, <c>.eps.norm1               the two LayerNorms' eps
    <c>.cpe.1.weight ... <c>.qkv.bias        float32 parameters
    <c>.out.feat, <c>.out.qkv, <c>.grad.<tensor>    float64 results: the features after the first residual add, the
                                             projection, and the gradients of feat, conv and the eight parameters.  Their low
                                             24 mantissa bits are cleared (2^-28 of the value, three orders below err32):
                                             the file compresses to two thirds
    <c>.err32.<tensor>                       max|x32 - x64| / max|x64| of the reference's float32 run
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_ptv3_index_golden import ROOT, reference_module  # noqa: E402

CASES = {"c32": (150, 32), "c64": (65, 64)}  # rows, channels
PARAMS = ("cpe.1.weight", "cpe.1.bias", "cpe.2.weight", "cpe.2.bias", "norm1.weight", "norm1.bias", "qkv.weight", "qkv.bias")


def run(M, dtype, C, feat, conv, w_feat, w_qkv, params):
    cpe_tail = M.PointSequential(torch.nn.Linear(C, C), torch.nn.LayerNorm(C)).to(dtype)   # cpe[1], cpe[2]
    norm1 = M.PointSequential(torch.nn.LayerNorm(C)).to(dtype)
    attn = M.SerializedAttention(channels=C, num_heads=C // 16, patch_size=48, enable_flash=False).to(dtype)
    own = {"cpe.1.weight": cpe_tail[0].weight, "cpe.1.bias": cpe_tail[0].bias, "cpe.2.weight": cpe_tail[1].weight,
           "cpe.2.bias": cpe_tail[1].bias, "norm1.weight": norm1[0].weight, "norm1.bias": norm1[0].bias,
           "qkv.weight": attn.qkv.weight, "qkv.bias": attn.qkv.bias}
    with torch.no_grad():
        for name, value in params.items():
            own[name].copy_(torch.from_numpy(value).to(dtype))
    x = torch.from_numpy(feat).to(dtype).requires_grad_(True)
    s = torch.from_numpy(conv).to(dtype).requires_grad_(True)
    shortcut = x                               # Block.forward: shortcut = point.feat; point = self.cpe(point) ...
    point = M.Point(feat=s)                    # ... whose first module has left the convolution's output in point.feat
    point = cpe_tail(point)
    point.feat = shortcut + point.feat
    out_feat = point.feat                      # the second shortcut
    point = norm1(point)
    out_qkv = attn.qkv(point.feat)             # SerializedAttention.forward's projection
    ((out_feat * torch.from_numpy(w_feat).to(dtype)).sum() + (out_qkv * torch.from_numpy(w_qkv).to(dtype)).sum()).backward()
    res = {"out.feat": out_feat.detach().numpy(), "out.qkv": out_qkv.detach().numpy(), "grad.feat": x.grad.numpy(),
           "grad.conv": s.grad.numpy()}
    res.update({"grad." + name: own[name].grad.numpy() for name in PARAMS})
    return res, float(cpe_tail[1].eps), float(norm1[0].eps)


def shorten(x64):
    """float64 with the low 24 mantissa bits cleared."""
    return (np.ascontiguousarray(x64).view(np.uint64) & ~np.uint64((1 << 24) - 1)).view(np.float64)


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "models", "pt_v3.py")):
        raise SystemExit("usage: make_ptv3_block_front_golden.py <reference root> (the directory that holds models/pt_v3.py)")
    M = reference_module(sys.argv[1])
    rng = np.random.default_rng(20261020)
    blob = {}
    for case, (n, C) in CASES.items():
        f32 = lambda a: np.asarray(a).astype(np.float32)  # noqa: E731
        feat, conv = f32(rng.normal(size=(n, C))), f32(rng.normal(size=(n, C)))
        w_feat, w_qkv = f32(rng.normal(size=(n, C))), f32(rng.normal(size=(n, 3 * C)))
        params = {"cpe.1.weight": rng.normal(size=(C, C)) * C ** -0.5, "cpe.1.bias": 0.1 * rng.normal(size=C),
                  "cpe.2.weight": 1.0 + 0.5 * rng.normal(size=C), "cpe.2.bias": 0.1 * rng.normal(size=C),
                  "norm1.weight": 1.0 + 0.5 * rng.normal(size=C), "norm1.bias": 0.1 * rng.normal(size=C),
                  "qkv.weight": rng.normal(size=(3 * C, C)) * C ** -0.5, "qkv.bias": 0.1 * rng.normal(size=3 * C)}
        params = {k: f32(v) for k, v in params.items()}
        r64, eps_cpe, eps_norm1 = run(M, torch.float64, C, feat, conv, w_feat, w_qkv, params)
        r32, _, _ = run(M, torch.float32, C, feat, conv, w_feat, w_qkv, params)
        blob.update({"%s.feat" % case: feat, "%s.conv" % case: conv, "%s.w.feat" % case: w_feat, "%s.w.qkv" % case: w_qkv,
                     "%s.eps.cpe" % case: np.asarray(eps_cpe), "%s.eps.norm1" % case: np.asarray(eps_norm1)})
        blob.update({"%s.%s" % (case, k): v for k, v in params.items()})
        for name, x64 in r64.items():
            assert x64.dtype == np.float64 and r32[name].dtype == np.float32
            blob["%s.%s" % (case, name)] = shorten(x64)
            err = float(np.abs(r32[name].astype(np.float64) - x64).max() / np.abs(x64).max())
            blob["%s.err32.%s" % (case, name)] = np.asarray(err)
            print(case, name, "float32 run: %.2e of the maximum" % err)
    path = os.path.join(ROOT, "tests", "golden", "ptv3_block_front.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes,", len(blob), "arrays")


if __name__ == "__main__":
    main()
