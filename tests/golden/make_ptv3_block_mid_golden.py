#!/usr/bin/env python
"""Generates tests/golden/ptv3_block_mid.npz with the REFERENCE's own models/pt_v3.py, imported on the CPU: what
Block.forward (pre_norm) runs between its first residual add and its feed-forward tail -- SerializedAttention.forward
(enable_flash=False, patch 48: the qkv projection, the gather into padded patches, the attention, the scatter back, the
output projection and proj_drop) followed by `shortcut + point.feat` -- run twice per case on the same seeded parameters
and inputs, once in float64 (the target) and once in float32 (the reference's own error).  Run in the build container only
(the reference does not exist on the GPU box):

    python tests/golden/make_ptv3_block_mid_golden.py <reference root>

As make_ptv3_block_front_golden.py: the repository root goes first on sys.path, so that pt_v3.py's `spconv`, `flash_attn`
and `torch_scatter` are the drop-ins of this repository, and a dict with attribute access stands in for `addict`.  The
module is built with upcast_attention=False and upcast_softmax=False: its upcasts are `.float()`, which would round the
float64 run to float32; the float32 run computes what it computes with them.  Two batch elements of 90 and 60 points give
patches of 48 with 6 and 36 duplicate slots.  The fixture holds inputs, parameters and the reference's outputs -- data only.
Per case <c>:

    <c>.feat, <c>.shortcut                   float32 [150, C]: the attention's input (norm1's output) and the Block's shortcut
    <c>.offset, <c>.order, <c>.inverse       int64: the batch offsets (90, 150), a seeded serialization order that keeps
                                             the batch elements apart, and its inverse
    <c>.w                                    float32 weights of the loss (out * w).sum()
    <c>.qkv.weight ... <c>.proj.bias         float32 parameters
    <c>.out, <c>.grad.<tensor>               float64 results: shortcut + attention, and the gradients of feat, shortcut
                                             and the four parameters, their low 24 mantissa bits cleared
    <c>.err32.<tensor>                       max|x32 - x64| / max|x64| of the reference's float32 run
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_ptv3_block_front_golden import shorten  # noqa: E402
from make_ptv3_index_golden import ROOT, reference_module  # noqa: E402

COUNTS, PATCH = (90, 60), 48
CASES = {"c32": 32, "c64": 64}  # channels; heads of 16
PARAMS = ("qkv.weight", "qkv.bias", "proj.weight", "proj.bias")


def run(M, dtype, C, feat, shortcut, w, order, inverse, params):
    attn = M.SerializedAttention(channels=C, num_heads=C // 16, patch_size=PATCH, enable_flash=False, upcast_attention=False,
                                 upcast_softmax=False).to(dtype)
    own = {"qkv.weight": attn.qkv.weight, "qkv.bias": attn.qkv.bias, "proj.weight": attn.proj.weight, "proj.bias": attn.proj.bias}
    with torch.no_grad():
        for name, value in params.items():
            own[name].copy_(torch.from_numpy(value).to(dtype))
    x = torch.from_numpy(feat).to(dtype).requires_grad_(True)
    s = torch.from_numpy(shortcut).to(dtype).requires_grad_(True)
    point = M.Point(feat=x, offset=torch.tensor(COUNTS).cumsum(0), serialized_order=torch.from_numpy(order)[None],
                    serialized_inverse=torch.from_numpy(inverse)[None])
    point = attn(point)                        # Block.forward: point = self.drop_path(self.attn(point)), drop_path an Identity
    assert attn.patch_size == PATCH and point["pad"].shape[0] == 192
    out = s + point.feat                       # point.feat = shortcut + point.feat
    (out * torch.from_numpy(w).to(dtype)).sum().backward()
    res = {"out": out.detach().numpy(), "grad.feat": x.grad.numpy(), "grad.shortcut": s.grad.numpy()}
    res.update({"grad." + name: own[name].grad.numpy() for name in PARAMS})
    return res


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "models", "pt_v3.py")):
        raise SystemExit("usage: make_ptv3_block_mid_golden.py <reference root> (the directory that holds models/pt_v3.py)")
    M = reference_module(sys.argv[1])
    rng = np.random.default_rng(20261021)
    n, blob = sum(COUNTS), {}
    for case, C in CASES.items():
        f32 = lambda a: np.asarray(a).astype(np.float32)  # noqa: E731
        feat, shortcut, w = (f32(rng.normal(size=(n, C))) for _ in range(3))
        order = np.concatenate([rng.permutation(c) + o for c, o in zip(COUNTS, (0, COUNTS[0]))]).astype(np.int64)
        inverse = np.empty_like(order)
        inverse[order] = np.arange(n)
        params = {"qkv.weight": rng.normal(size=(3 * C, C)) * C ** -0.5, "qkv.bias": 0.1 * rng.normal(size=3 * C),
                  "proj.weight": rng.normal(size=(C, C)) * C ** -0.5, "proj.bias": 0.1 * rng.normal(size=C)}
        params = {k: f32(v) for k, v in params.items()}
        r64 = run(M, torch.float64, C, feat, shortcut, w, order, inverse, params)
        r32 = run(M, torch.float32, C, feat, shortcut, w, order, inverse, params)
        blob.update({"%s.feat" % case: feat, "%s.shortcut" % case: shortcut, "%s.w" % case: w, "%s.order" % case: order,
                     "%s.inverse" % case: inverse, "%s.offset" % case: np.cumsum(COUNTS).astype(np.int64)})
        blob.update({"%s.%s" % (case, k): v for k, v in params.items()})
        for name, x64 in r64.items():
            assert x64.dtype == np.float64 and r32[name].dtype == np.float32
            blob["%s.%s" % (case, name)] = shorten(x64)
            err = float(np.abs(r32[name].astype(np.float64) - x64).max() / np.abs(x64).max())
            blob["%s.err32.%s" % (case, name)] = np.asarray(err)
            print(case, name, "float32 run: %.2e of the maximum" % err)
    path = os.path.join(ROOT, "tests", "golden", "ptv3_block_mid.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes,", len(blob), "arrays")


if __name__ == "__main__":
    main()
