#!/usr/bin/env python
"""Generates tests/golden/ptv3_index.npz with the REFERENCE's own models/pt_v3.py, imported on the CPU: the codes of
Serializator.encode and the plans of SerializedAttention.get_padding_and_inverse.  Run in the build container only (the
reference does not exist on the GPU box):

    python tests/golden/make_ptv3_index_golden.py <reference root>

The repository root goes first on sys.path, so that pt_v3.py's `spconv`, `flash_attn` and `torch_scatter` are the
drop-ins of this repository; `addict` is not installed, a dict with attribute access stands in for it.  The fixture holds
inputs and the reference's outputs -- data only.  The order of equal codes is NOT recorded: torch.argsort leaves it open.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ORDERS = ("cord", "z", "z-trans", "hilbert", "hilbert-trans")
DEPTHS = (1, 5, 8, 11, 16)
N = 97
COUNTS = {"p4": ([5, 3, 9, 4, 8, 1, 17], 4), "p1024": ([1024, 1, 1025, 2047, 2048, 3], 1024), "p16": ([7], 16),
          "p32": ([33, 64, 65], 32), "one": ([1], 8), "zero": ([6, 0, 11, 4], 4)}


class _Dict(dict):
    """What pt_v3.py needs of addict.Dict: keys as attributes."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


def reference_module(ref_root):
    sys.path.insert(0, ROOT)
    sys.modules.setdefault("addict", types.SimpleNamespace(Dict=_Dict))
    sys.path.append(ref_root)
    import models.pt_v3 as M
    return M


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "models", "pt_v3.py")):
        raise SystemExit("usage: make_ptv3_index_golden.py <reference root> (the directory that holds models/pt_v3.py)")
    M = reference_module(sys.argv[1])
    S = M.Serializator()
    rng = np.random.default_rng(20240515)
    blob = {}
    for depth in DEPTHS:
        # coordinates over the whole cube of the depth, its corners included, and a few equal rows
        g = rng.integers(0, 1 << depth, (N, 3)).astype(np.int32)
        g[0], g[1], g[2] = 0, (1 << depth) - 1, g[3]
        b = np.sort(rng.integers(0, 5, N)).astype(np.int64)
        blob["d%d.grid" % depth], blob["d%d.batch" % depth] = g, b
        for with_batch in (0, 1):
            code = [S.encode(torch.from_numpy(g), 0.01, torch.from_numpy(b) if with_batch else None, depth, order=o)
                    for o in ORDERS]
            blob["d%d.code.%d" % (depth, with_batch)] = torch.stack(code).numpy()
    # cord at a grid size where dividing and multiplying by the reciprocal differ, coordinates up to 511
    g = rng.integers(0, 512, (N, 3)).astype(np.int32)
    g[0], g[1] = 0, 511
    blob["cord003.grid"] = g
    blob["cord003.code"] = S.encode(torch.from_numpy(g), 0.003, None, 9, order="cord").numpy()[None]
    # every coordinate below 256 on each axis at grid size 0.01: the division, element by element
    a = np.arange(256, dtype=np.int32)
    g = np.concatenate([np.stack([a, 0 * a, 0 * a], 1), np.stack([0 * a, a, 0 * a], 1), np.stack([a, a[::-1], a], 1)])
    blob["cord256.grid"] = g
    blob["cord256.code"] = S.encode(torch.from_numpy(g), 0.01, None, 8, order="cord").numpy()[None]
    att = M.SerializedAttention.__new__(M.SerializedAttention)
    for name, (counts, patch) in COUNTS.items():
        att.patch_size = patch
        point = _Dict(offset=torch.tensor(np.cumsum(counts), dtype=torch.long))
        pad, unpad, cu = M.SerializedAttention.get_padding_and_inverse(att, point)
        assert pad.dtype == torch.int64 and unpad.dtype == torch.int64 and cu.dtype == torch.int32
        blob["%s.counts" % name] = np.asarray(counts, np.int64)
        blob["%s.patch" % name] = np.asarray(patch, np.int64)
        blob["%s.pad" % name], blob["%s.unpad" % name], blob["%s.cu" % name] = pad.numpy(), unpad.numpy(), cu.numpy()
    path = os.path.join(ROOT, "tests", "golden", "ptv3_index.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes,", len(blob), "arrays")


if __name__ == "__main__":
    main()
