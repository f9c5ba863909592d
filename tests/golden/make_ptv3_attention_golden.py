#!/usr/bin/env python
"""Generates tests/golden/ptv3_attention.npz with the REFERENCE's own models/pt_v3.py, imported on the CPU: its
SerializedAttention(channels=32, num_heads=2, enable_flash=False, upcast_attention=False, upcast_softmax=False) -- the
default, non-flash branch -- run twice per case on the same seeded parameters and inputs, once in float64 (the target)
and once in float32 (the reference's own error).  Run in the build container only (the reference does not exist on the
GPU box):

    python tests/golden/make_ptv3_attention_golden.py <reference root>

As make_ptv3_index_golden.py: the repository root goes first on sys.path, so that pt_v3.py's `spconv`, `flash_attn` and
`torch_scatter` are the drop-ins of this repository, and a dict with attribute access stands in for `addict`.  The
fixture holds inputs, parameters and the reference's outputs -- data only.  Per case <c>:

    <c>.counts, <c>.patch, <c>.K             rows per batch element, the module's patch_size, the patch size it chose
    <c>.feat, <c>.order, <c>.inverse, <c>.w  float32 features [n, 32], the serialized order and its inverse [1, n], and
                                             the weights of the loss (out * w).sum()
    <c>.qkv.weight ... <c>.proj.bias         float32 parameters
    <c>.out, <c>.grad.<tensor>               float64 results: the output features and the gradients of feat and of the
                                             four parameters
    <c>.err32.<tensor>                       max|x32 - x64| / max|x64| of the reference's float32 run
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_ptv3_index_golden import ROOT, _Dict, reference_module  # noqa: E402

CHANNELS, HEADS = 32, 2
CASES = {"k37": ([100, 37, 64], 1024), "k64": ([150, 64, 200], 64), "k16": ([16], 16)}
PARAMS = ("qkv.weight", "qkv.bias", "proj.weight", "proj.bias")


def run(M, dtype, counts, patch, feat, order, inverse, w, params):
    att = M.SerializedAttention(channels=CHANNELS, num_heads=HEADS, patch_size=patch, enable_flash=False,
                                upcast_attention=False, upcast_softmax=False).to(dtype)
    with torch.no_grad():
        for name, value in params.items():
            att.get_parameter(name).copy_(torch.from_numpy(value).to(dtype))
    x = torch.from_numpy(feat).to(dtype).requires_grad_(True)
    point = _Dict(feat=x, offset=torch.tensor(np.cumsum(counts), dtype=torch.long),
                  serialized_order=torch.from_numpy(order), serialized_inverse=torch.from_numpy(inverse))
    out = att(point).feat
    (out * torch.from_numpy(w).to(dtype)).sum().backward()
    res = {"out": out.detach().numpy(), "grad.feat": x.grad.numpy()}
    res.update({"grad." + name: att.get_parameter(name).grad.numpy() for name in PARAMS})
    return res, int(att.patch_size)


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "models", "pt_v3.py")):
        raise SystemExit("usage: make_ptv3_attention_golden.py <reference root> (the directory that holds models/pt_v3.py)")
    M = reference_module(sys.argv[1])
    rng = np.random.default_rng(20241019)
    blob = {}
    for case, (counts, patch) in CASES.items():
        n = int(np.sum(counts))
        # a permutation inside every batch element, as a serialization gives
        order = np.concatenate([lo + rng.permutation(c) for lo, c in zip(np.cumsum([0] + counts[:-1]), counts)])
        inverse = np.empty_like(order)
        inverse[order] = np.arange(n)
        feat = rng.normal(size=(n, CHANNELS)).astype(np.float32)
        w = rng.normal(size=(n, CHANNELS)).astype(np.float32)
        params = {"qkv.weight": rng.normal(size=(3 * CHANNELS, CHANNELS)) * CHANNELS ** -0.5,
                  "qkv.bias": rng.normal(size=3 * CHANNELS) * 0.1,
                  "proj.weight": rng.normal(size=(CHANNELS, CHANNELS)) * CHANNELS ** -0.5,
                  "proj.bias": rng.normal(size=CHANNELS) * 0.1}
        params = {k: v.astype(np.float32) for k, v in params.items()}
        args = (counts, patch, feat, order[None].astype(np.int64), inverse[None].astype(np.int64), w, params)
        r64, K = run(M, torch.float64, *args)
        r32, K32 = run(M, torch.float32, *args)
        assert K == K32 == min(min(counts), patch)
        blob.update({"%s.counts" % case: np.asarray(counts, np.int64), "%s.patch" % case: np.asarray(patch, np.int64),
                     "%s.K" % case: np.asarray(K, np.int64), "%s.feat" % case: feat, "%s.order" % case: args[3],
                     "%s.inverse" % case: args[4], "%s.w" % case: w})
        blob.update({"%s.%s" % (case, k): v for k, v in params.items()})
        for name, x64 in r64.items():
            assert x64.dtype == np.float64 and r32[name].dtype == np.float32
            blob["%s.%s" % (case, name)] = x64
            err = float(np.abs(r32[name].astype(np.float64) - x64).max() / np.abs(x64).max())
            blob["%s.err32.%s" % (case, name)] = np.asarray(err)
            print(case, "K", K, name, "float32 run: %.2e of the maximum" % err)
    path = os.path.join(ROOT, "tests", "golden", "ptv3_attention.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes,", len(blob), "arrays")


if __name__ == "__main__":
    main()
