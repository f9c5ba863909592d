#!/usr/bin/env python
"""Generates tests/golden/ptv3_pool.npz with the REFERENCE's own models/pt_v3.py, imported on the CPU: a
SerializedPooling + SerializedUnpooling pair, run in float64 and again in float32.  Run in the build container only (the
reference does not exist on the GPU box):

    python tests/golden/make_ptv3_pool_golden.py <reference root>

The repository root goes first on sys.path, so that pt_v3.py's `spconv` and `flash_attn` are the drop-ins of this
repository; `addict` is not installed, a dict with attribute access stands in for it; this repository's torch_scatter runs
on the GPU only, so a few lines of torch ops stand in for its segment_csr while the fixture is recorded.  The fixture
holds data only: the inputs, the module weights, every integer key of the pooled point set, and per float tensor (feat,
coord, the unpooled feat, the gradients of the input features and of every parameter for a fixed dout) the float64 value
and `err32`, the distance of the reference's own float32 run from it as a fraction of the tensor's maximum (`scale`) -- the
scheme of ptv3_attr_head.npz.  Modules are in training mode (BatchNorm1d takes the batch's statistics), shuffle_orders is off, and the reference's sorts
run with stable=True (see _stable_sorts).
"""
import functools
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N, BATCHES, C_IN, C_POOL, C_UP = 333, 3, 20, 36, 12
CASES = {  # name: (orders, grid_size, coordinate range, stride, reduce)
    "a": (("z", "z-trans", "hilbert"), 0.01, 32, 2, "max"),
    "b": (("cord",), 0.01, 32, 2, "max"),
    "c": (("z", "z-trans", "hilbert"), 0.01, 4, 8, "mean"),
}


class _Dict(dict):
    """What pt_v3.py needs of addict.Dict: keys as attributes."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


def _segment_csr(src, indptr, out=None, reduce="sum"):
    """torch_scatter.segment_csr along dim 0 in torch ops; min and max route the gradient to the first row attaining."""
    s = indptr.numel() - 1
    counts = indptr[1:] - indptr[:-1]
    seg = torch.repeat_interleave(torch.arange(s), counts)
    if reduce in ("sum", "add", "mean"):
        res = torch.zeros((s,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, seg, src[: seg.numel()])
        return res / counts.clamp(min=1).to(src.dtype).unsqueeze(-1) if reduce == "mean" else res
    arg = torch.zeros((s,) + tuple(src.shape[1:]), dtype=torch.long)
    with torch.no_grad():
        for c in range(s):
            lo, hi = int(indptr[c]), int(indptr[c + 1])
            assert hi > lo
            v = src[lo:hi]
            arg[c] = lo + (v.argmax(0) if reduce == "max" else v.argmin(0))
    return torch.gather(src, 0, arg)


class _stable_sorts:
    """torch.sort and torch.argsort with stable=True while the reference runs.  Upstream leaves the order of equal keys
    open, and this torch build's CPU sort does not keep it (333 int64 keys come back in another order than with
    stable=True); every tie order is a run of the reference, and the fixture records the one with ties to the lower row."""

    def __enter__(self):
        self.own = (torch.sort, torch.argsort)
        torch.sort = functools.partial(self.own[0], stable=True)
        torch.argsort = functools.partial(self.own[1], stable=True)

    def __exit__(self, *exc):
        torch.sort, torch.argsort = self.own


def reference_module(ref_root):
    sys.path.insert(0, ROOT)
    sys.modules.setdefault("addict", types.SimpleNamespace(Dict=_Dict))
    sys.modules["torch_scatter"] = types.SimpleNamespace(segment_csr=_segment_csr)
    sys.path.append(ref_root)
    import models.pt_v3 as M
    return M


def run(M, case, shared, weights, dtype):
    orders, grid_size, _, stride, reduce = CASES[case]
    bn = functools.partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01)  # as PointTransformerV3 builds it
    pool = M.SerializedPooling(C_IN, C_POOL, stride=stride, norm_layer=bn, act_layer=torch.nn.GELU, reduce=reduce,
                               shuffle_orders=False, traceable=True)
    unpool = M.SerializedUnpooling(C_POOL, C_IN, C_UP, norm_layer=bn, act_layer=torch.nn.GELU)
    for name, module in (("pool", pool), ("unpool", unpool)):
        if weights.get(name) is None:
            weights[name] = {k: v.detach().clone() for k, v in module.state_dict().items()}
        module.load_state_dict(weights[name])
        module.to(dtype).train()
    feat = shared["feat"].to(dtype).requires_grad_(True)
    point = M.Point(feat=feat, coord=shared["coord"].to(dtype), grid_coord=shared[case + ".grid"], batch=shared["batch"],
                    grid_size=grid_size)
    point.serialization(order=list(orders), shuffle_orders=False)
    ints = {"in." + k: point[k].clone() for k in ("serialized_code", "serialized_order", "serialized_inverse")}
    ints["in.serialized_depth"] = torch.tensor(point.serialized_depth)
    pooled = pool(point)
    for k in ("grid_coord", "serialized_code", "serialized_order", "serialized_inverse", "batch", "pooling_inverse", "offset"):
        ints[k] = pooled[k].clone()
    ints["serialized_depth"] = torch.tensor(pooled.serialized_depth)
    floats = {"feat": pooled.feat, "coord": pooled.coord}
    parent = unpool(pooled)
    floats["unpooled"] = parent.feat
    params = [("pool." + k, p) for k, p in pool.named_parameters()] + [("unpool." + k, p) for k, p in unpool.named_parameters()]
    grads = torch.autograd.grad((parent.feat * shared["dout"].to(dtype)).sum(), [feat] + [p for _, p in params])
    floats["grad.feat"] = grads[0]
    for (name, _), g in zip(params, grads[1:]):
        floats["grad." + name] = g
    return ints, {k: v.detach().double().numpy() for k, v in floats.items()}


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "models", "pt_v3.py")):
        raise SystemExit("usage: make_ptv3_pool_golden.py <reference root> (the directory that holds models/pt_v3.py)")
    M = reference_module(sys.argv[1])
    rng = np.random.default_rng(20240611)
    torch.manual_seed(20240611)
    shared = {"feat": torch.from_numpy(rng.standard_normal((N, C_IN)).astype(np.float32)),
              "coord": torch.from_numpy(rng.uniform(0, 0.32, (N, 3)).astype(np.float32)),
              "batch": torch.from_numpy(np.sort(rng.integers(0, BATCHES, N)).astype(np.int64)),
              "dout": torch.from_numpy(rng.standard_normal((N, C_UP)).astype(np.float32))}
    blob = {k: v.numpy() for k, v in shared.items()}
    weights = {}
    for case, (orders, grid_size, extent, stride, reduce) in CASES.items():
        # a dozen occupied cells of twice the stride (or thirty voxels), several rows in most clusters, some rows in one
        # voxel, in no order
        if extent > 4:
            cells = rng.integers(0, extent // 4, (12, 3)) * 4
            g = (cells[rng.integers(0, 12, N)] + rng.integers(0, 4, (N, 3))).astype(np.int32)
        else:
            g = rng.integers(0, extent, (30, 3))[rng.integers(0, 30, N)].astype(np.int32)
        g[0], g[1] = 0, extent - 1
        shared[case + ".grid"] = torch.from_numpy(g)
        blob[case + ".grid"] = g
        blob[case + ".orders"] = np.array(orders)
        blob[case + ".grid_size"], blob[case + ".stride"], blob[case + ".reduce"] = np.float64(grid_size), np.int64(stride), np.array(reduce)
        with _stable_sorts():
            ints, want = run(M, case, shared, weights, torch.float64)
            ints32, got = run(M, case, shared, weights, torch.float32)
        for k, v in ints.items():
            assert torch.equal(v, ints32[k]), k
            blob["%s.int.%s" % (case, k)] = v.numpy()
        for k, v in want.items():
            # a bias in front of a BatchNorm1d in training mode has the gradient 0, and what is left of it is rounding
            # noise: a bias gradient is measured against the larger of its own maximum and its weight's
            scale = max(np.abs(v).max(), np.abs(want[k[:-4] + "weight"]).max() if k.endswith(".bias") else 0.0)
            blob["%s.%s" % (case, k)] = v
            blob["%s.scale.%s" % (case, k)] = np.float64(scale)
            blob["%s.err32.%s" % (case, k)] = np.float64(np.abs(got[k] - v).max() / scale)
        print(case, "rows", N, "clusters", int(ints["batch"].numel()), "pooled depth", int(ints["serialized_depth"]),
              "worst err32 %.2e" % max(float(blob["%s.err32.%s" % (case, k)]) for k in want))
    for name, state in weights.items():
        for k, v in state.items():
            blob["w.%s.%s" % (name, k)] = v.numpy()
    path = os.path.join(ROOT, "tests", "golden", "ptv3_pool.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes,", len(blob), "arrays")


if __name__ == "__main__":
    main()
