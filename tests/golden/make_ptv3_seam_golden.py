#!/usr/bin/env python
"""Generates tests/golden/ptv3_seam.npz with the REFERENCE's own models/pt_v3.py, imported on the CPU the way
make_ptv3_pool_golden.py imports it: one SerializedPooling + SerializedUnpooling pair and one
PointSequential(Linear, BatchNorm1d, GELU) on a Point, run in float64 and again in float32.  Run in the build container
only (the reference does not exist on the GPU box):

    python tests/golden/make_ptv3_seam_golden.py <reference root>

Case (a) is training mode from the recorded initial state; case (b) is eval mode after that one training step (the running
statistics are then the ones step (a) left).  The fixture holds data only: the inputs, the module weights, the integer keys
of the pooled point set and the counters, and per float tensor (the pooled and the unpooled feat, the container's output,
the gradients of the two input features and of every parameter for fixed dout, the running statistics after the step) the
float64 value and `err32`, the distance of the reference's own float32 run from it as a fraction of `scale` -- the scheme
of ptv3_pool.npz: a bias gradient is measured against the larger of its own maximum and its weight's, a buffer against its
own maximum.  shuffle_orders is off and the reference's sorts run with stable=True, for the reason DESIGN.md section 15.6
gives.
"""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_ptv3_pool_golden import ROOT, _stable_sorts, reference_module  # noqa: E402

N, BATCHES, C_IN, C_POOL, C_UP, C_SEQ = 333, 3, 20, 36, 12, 28
ORDERS, GRID_SIZE, EXTENT, STRIDE, REDUCE = ("z", "z-trans", "hilbert"), 0.01, 32, 2, "max"


def build(M, weights, dtype):
    bn = functools.partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01)  # as PointTransformerV3 builds it
    pool = M.SerializedPooling(C_IN, C_POOL, stride=STRIDE, norm_layer=bn, act_layer=torch.nn.GELU, reduce=REDUCE,
                               shuffle_orders=False, traceable=True)
    unpool = M.SerializedUnpooling(C_POOL, C_IN, C_UP, norm_layer=bn, act_layer=torch.nn.GELU)
    seq = M.PointSequential(torch.nn.Linear(C_IN, C_SEQ))
    seq.add(bn(C_SEQ))
    seq.add(torch.nn.GELU())
    mods = {"pool": pool, "unpool": unpool, "seq": seq}
    for name, module in mods.items():
        if weights.get(name) is None:
            weights[name] = {k: v.detach().clone() for k, v in module.state_dict().items()}
        module.load_state_dict(weights[name])
        module.to(dtype)
    return mods


def step(M, mods, shared, dtype, training):
    for module in mods.values():
        module.train(training)
        module.zero_grad()
    feat = shared["feat"].to(dtype).clone().requires_grad_(True)       # (two leaves: .to() of the same dtype is no copy)
    feat_seq = shared["feat"].to(dtype).clone().requires_grad_(True)
    common = dict(coord=shared["coord"].to(dtype), grid_coord=shared["grid"], batch=shared["batch"], grid_size=GRID_SIZE)
    point = M.Point(feat=feat, **common)
    point.serialization(order=list(ORDERS), shuffle_orders=False)
    ints = {"in." + k: point[k].clone() for k in ("serialized_code", "serialized_order", "serialized_inverse")}
    ints["in.serialized_depth"] = torch.tensor(point.serialized_depth)
    pooled = mods["pool"](point)
    for k in ("grid_coord", "serialized_code", "serialized_order", "serialized_inverse", "batch", "pooling_inverse"):
        ints[k] = pooled[k].clone()
    ints["serialized_depth"] = torch.tensor(pooled.serialized_depth)
    floats = {"pooled": pooled.feat}
    parent = mods["unpool"](pooled)
    floats["unpooled"] = parent.feat
    out = mods["seq"](M.Point(feat=feat_seq, **common))
    floats["seq"] = out.feat
    params = [("%s.%s" % (name, k), p) for name, module in mods.items() for k, p in module.named_parameters()]
    loss = (parent.feat * shared["dout"].to(dtype)).sum() + (out.feat * shared["dseq"].to(dtype)).sum()
    grads = torch.autograd.grad(loss, [feat, feat_seq] + [p for _, p in params])
    floats["grad.feat"], floats["grad.feat_seq"] = grads[0], grads[1]
    for (name, _), g in zip(params, grads[2:]):
        floats["grad." + name] = g
    for name, module in mods.items():
        for k, b in module.named_buffers():
            if b.dtype == torch.int64:
                ints["buf.%s.%s" % (name, k)] = b.clone()
            elif training:   # eval mode leaves the running statistics as they are: nothing to measure
                floats["buf.%s.%s" % (name, k)] = b.clone()
    return ints, {k: v.detach().double().numpy() for k, v in floats.items()}


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "models", "pt_v3.py")):
        raise SystemExit("usage: make_ptv3_seam_golden.py <reference root> (the directory that holds models/pt_v3.py)")
    M = reference_module(sys.argv[1])
    rng = np.random.default_rng(20261020)
    torch.manual_seed(20261020)
    cells = rng.integers(0, EXTENT // 4, (12, 3)) * 4
    g = (cells[rng.integers(0, 12, N)] + rng.integers(0, 4, (N, 3))).astype(np.int32)
    g[0], g[1] = 0, EXTENT - 1
    shared = {"feat": torch.from_numpy(rng.standard_normal((N, C_IN)).astype(np.float32)),
              "coord": torch.from_numpy(rng.uniform(0, 0.32, (N, 3)).astype(np.float32)),
              "batch": torch.from_numpy(np.sort(rng.integers(0, BATCHES, N)).astype(np.int64)),
              "dout": torch.from_numpy(rng.standard_normal((N, C_UP)).astype(np.float32)),
              "dseq": torch.from_numpy(rng.standard_normal((N, C_SEQ)).astype(np.float32)),
              "grid": torch.from_numpy(g)}
    blob = {k: v.numpy() for k, v in shared.items()}
    blob["orders"], blob["grid_size"], blob["stride"], blob["reduce"] = np.array(ORDERS), np.float64(GRID_SIZE), np.int64(STRIDE), np.array(REDUCE)
    weights = {}
    with _stable_sorts():
        m64, m32 = build(M, weights, torch.float64), build(M, weights, torch.float32)
        for case, training in (("a", True), ("b", False)):   # (b) runs on the state (a) left
            ints, want = step(M, m64, shared, torch.float64, training)
            ints32, got = step(M, m32, shared, torch.float32, training)
            for k, v in ints.items():
                assert torch.equal(v, ints32[k]), k
                blob["%s.int.%s" % (case, k)] = v.numpy()
            for k, v in want.items():
                scale = max(np.abs(v).max(), np.abs(want[k[:-4] + "weight"]).max() if k.endswith(".bias") and k.startswith("grad.") else 0.0)
                blob["%s.%s" % (case, k)] = v
                blob["%s.scale.%s" % (case, k)] = np.float64(scale)
                blob["%s.err32.%s" % (case, k)] = np.float64(np.abs(got[k] - v).max() / scale)
            print(case, "rows", N, "clusters", int(ints["batch"].numel()),
                  "worst err32 %.2e" % max(float(blob["%s.err32.%s" % (case, k)]) for k in want),
                  "smallest err32 %.2e" % min(float(blob["%s.err32.%s" % (case, k)]) for k in want))
    for name, state in weights.items():
        for k, v in state.items():
            blob["w.%s.%s" % (name, k)] = v.numpy()
    path = os.path.join(ROOT, "tests", "golden", "ptv3_seam.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes,", len(blob), "arrays")


if __name__ == "__main__":
    main()
