#!/usr/bin/env python
"""Generates tests/golden/attr_head_plain.npz with the REFERENCE's own models/generator.py, imported on the CPU: its
GaussianAttrMLP built with z_dim=None (the background generator: every layer a plain Linear) and run with zs=None, twice
per case on the same seeded parameters and inputs, once in float64 (the target) and once in float32 (the reference's own
error).  Run in the build container only (the reference does not exist on the GPU box):

    python tests/golden/make_attr_head_plain_golden.py <reference root>

The loader and the layout are make_attr_head_golden.py's; what differs is the module (no style codes, so no ids and no z)
and the cases.  The fixture holds inputs, parameters and the reference's outputs -- data only.  Per case <c>:

    <c>.n_shared, <c>.layers, <c>.factors   n_shared_layers; n_layers and factors of xyz, rgb, scale, opacity (-1: the
                                            key is absent)
    <c>.pt_feat, <c>.onehots                float32 inputs [1, n, 24] and [1, n, 7]
    <c>.w.<key>                             the weights of the loss: sum over the keys of (out[key] * w).sum()
    <c>.param.<name>                        float32 parameters
    <c>.out.<key>, <c>.grad.pt_feat, <c>.grad.<name>    float64 results
    <c>.err32.<the same names>              max|x32 - x64| / max|x64| of the reference's float32 run

The float32 run of some tensor can agree with float64 to better than float32 rounds (a sum that happens to land on the
nearest float): its err32 would set a bar, 4 x err32, under one float32 unit of the tensor's maximum, which no float32
summation in another order can be held to.  So the data seed is the first from SEED on at which every err32 is at least
2^-25 (4 x err32 is then at least one unit, 2^-23); the seeds passed over and their tensors are printed.

A parameter the reference never uses (upstream applies every one of a key's layers to the shared activation, so only the
last reaches the output layer) has no gradient there; it is stored without one and the test expects none.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_attr_head_golden import CLASSES, HIDDEN, IN_DIM, KEYS, ROOT, reference_module  # noqa: E402

# n_shared_layers, n_layers and factors per key, rows
CASES = {
    "a": (1, {"rgb": 1}, {"rgb": 2.0}, 200),
    "b": (2, {"xyz": 1, "rgb": 2, "scale": 0, "opacity": 1}, {"xyz": 0.75, "rgb": 2.0, "scale": 0.5, "opacity": 0.6}, 333),
}


def run(M, dtype, case, data, params):
    n_shared, layers, factors, n = CASES[case]
    torch.set_default_dtype(dtype)
    try:
        head = M.GaussianAttrMLP(CLASSES, IN_DIM, None, HIDDEN, n_shared, factors=dict(factors), n_layers=dict(layers)).to(dtype)
        with torch.no_grad():
            for name, value in params.items():
                head.get_parameter(name).copy_(torch.from_numpy(value).to(dtype))
        x = torch.from_numpy(data["pt_feat"]).to(dtype).requires_grad_(True)
        out = head(x, torch.from_numpy(data["onehots"]).to(dtype), None)
        assert list(out) == list(factors)
        sum((out[k] * torch.from_numpy(data["w." + k]).to(dtype)).sum() for k in factors).backward()
        res = {"out." + k: v.detach().numpy() for k, v in out.items()}
        res["grad.pt_feat"] = x.grad.numpy()
        res.update({"grad." + name: p.grad.numpy() for name, p in head.named_parameters() if p.grad is not None})
        return res
    finally:
        torch.set_default_dtype(torch.float32)


SEED, FLOOR = 20261021, 2.0 ** -25


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "models", "generator.py")):
        raise SystemExit("usage: make_attr_head_plain_golden.py <reference root> (the directory that holds models/generator.py)")
    M = reference_module(sys.argv[1])
    for seed in range(SEED, SEED + 64):
        blob = cases(M, seed)
        lucky = sorted(k for k, v in blob.items() if ".err32." in k and float(v) < FLOOR)
        if not lucky:
            break
        print("seed %d passed over: the float32 run is closer than float32 rounds on" % seed, lucky)
    else:
        raise SystemExit("no seed in 64 with every err32 at least 2^-25")
    blob["seed"] = np.asarray(seed, np.int64)
    path = os.path.join(ROOT, "tests", "golden", "attr_head_plain.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes,", len(blob), "arrays, seed", seed)


def cases(M, seed):
    rng = np.random.default_rng(seed)
    blob = {}
    for case, (n_shared, layers, factors, n) in CASES.items():
        torch.manual_seed(11)
        head = M.GaussianAttrMLP(CLASSES, IN_DIM, None, HIDDEN, n_shared, factors=dict(factors), n_layers=dict(layers))
        params = {name: p.detach().numpy().copy() for name, p in head.named_parameters()}
        for name in params:  # the initial output layers are small: move them
            if name.startswith("fc_out_"):
                params[name] = params[name] + rng.normal(size=params[name].shape).astype(np.float32) * 0.3
        if "scale" in factors:
            params["fc_out_scale.weight"] = params["fc_out_scale.weight"] * 3.0
        data = {"pt_feat": rng.normal(size=(1, n, IN_DIM)).astype(np.float32),
                "onehots": np.eye(CLASSES, dtype=np.float32)[rng.integers(0, CLASSES, size=n)][None]}
        for k in factors:
            data["w." + k] = rng.normal(size=(1, n, 1 if k == "opacity" else 3)).astype(np.float32)
        r64, r32 = run(M, torch.float64, case, data, params), run(M, torch.float32, case, data, params)
        if "scale" in factors:  # the clamp must be active on some rows and inactive on others
            raw = (r64["out.scale"][0] - 1.0) / factors["scale"]
            clamped = np.isclose(np.abs(raw), 1.0, rtol=0, atol=1e-12)
            assert clamped.any() and (~clamped).any(), (int(clamped.sum()), clamped.size)
            print(case, "scale: %d of %d values clamped" % (int(clamped.sum()), clamped.size))
        unused = sorted(name for name in params if "grad." + name not in r64)
        for name in unused:  # fc_<n>_<key>_<i>.<weight or bias>, and never a key's last layer
            _, _, key, i = name.split(".")[0].split("_")
            assert int(i) < layers[key] - 1, name
        print(case, "parameters the reference does not use:", unused)
        blob["%s.n_shared" % case] = np.asarray(n_shared, np.int64)
        blob["%s.layers" % case] = np.asarray([layers.get(k, -1) for k in KEYS], np.int64)
        blob["%s.factors" % case] = np.asarray([factors.get(k, -1.0) for k in KEYS], np.float64)
        blob.update({"%s.%s" % (case, k): v for k, v in data.items()})
        blob.update({"%s.param.%s" % (case, k): v for k, v in params.items()})
        for name, x64 in r64.items():
            assert x64.dtype == np.float64 and r32[name].dtype == np.float32, (name, x64.dtype, r32[name].dtype)
            err = float(np.abs(r32[name].astype(np.float64) - x64).max() / np.abs(x64).max())
            assert err > 0, name
            blob["%s.%s" % (case, name)] = x64
            blob["%s.err32.%s" % (case, name)] = np.asarray(err)
    return blob


if __name__ == "__main__":
    main()
