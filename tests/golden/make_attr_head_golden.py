#!/usr/bin/env python
"""Generates tests/golden/attr_head.npz with the REFERENCE's own models/generator.py, imported on the CPU: its
GaussianAttrMLP run with a `zs` dict (one style code and one boolean mask per instance), twice per case on the same
seeded parameters and inputs, once in float64 (the target) and once in float32 (the reference's own error).  Run in the
build container only (the reference does not exist on the GPU box):

    python tests/golden/make_attr_head_golden.py <reference root>

generator.py is loaded by path; empty modules stand in for its two imports that the head does not use
(`extensions.grid_encoder`, `models.pt_v3`).  The method allocates its outputs with torch.zeros in the default dtype, so
the float64 run has torch.set_default_dtype(torch.float64) around it.  The fixture holds inputs, parameters and the
reference's outputs -- data only.  Per case <c>:

    <c>.n_shared, <c>.layers, <c>.factors   n_shared_layers; n_layers and factors of xyz, rgb, scale, opacity (-1: the
                                            key is absent)
    <c>.pt_feat, <c>.onehots                float32 inputs [1, n, 24] and [1, n, 7]
    <c>.ids, <c>.z                          int64 [n]: the row's instance in dict order, -1 without a style; float32
                                            codes [instances, 16]
    <c>.w.<key>                             the weights of the loss: sum over the keys of (out[key] * w).sum()
    <c>.param.<name>                        float32 parameters
    <c>.out.<key>, <c>.grad.pt_feat, <c>.grad.<name>    float64 results
    <c>.err32.<the same names>              max|x32 - x64| / max|x64| of the reference's float32 run
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KEYS = ("xyz", "rgb", "scale", "opacity")
HIDDEN, Z_DIM, IN_DIM, CLASSES = 48, 16, 24, 7
# n_shared_layers, n_layers and factors per key (None: the key is absent), rows, instances, rows without a style
CASES = {
    "a": (2, {"xyz": 1, "rgb": 2, "scale": 0, "opacity": 1}, {"xyz": 0.75, "rgb": 2.0, "scale": 0.5, "opacity": 0.6}, 333, 6, 5),
    "b": (1, {"rgb": 1}, {"rgb": 2.0}, 200, 1, 0),
}


def reference_module(ref_root):
    for name in ("extensions", "extensions.grid_encoder", "models", "models.pt_v3"):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location("reference_generator", os.path.join(ref_root, "models", "generator.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def run(M, dtype, case, data, params):
    n_shared, layers, factors, n, _, _ = CASES[case]
    torch.set_default_dtype(dtype)
    try:
        head = M.GaussianAttrMLP(CLASSES, IN_DIM, Z_DIM, HIDDEN, n_shared, factors=dict(factors), n_layers=dict(layers)).to(dtype)
        with torch.no_grad():
            for name, value in params.items():
                head.get_parameter(name).copy_(torch.from_numpy(value).to(dtype))
        x = torch.from_numpy(data["pt_feat"]).to(dtype).requires_grad_(True)
        ids = torch.from_numpy(data["ids"])
        zs = {100 + g: {"z": torch.from_numpy(data["z"][g:g + 1]).to(dtype), "idx": (ids == g).unsqueeze(0)}
              for g in range(data["z"].shape[0])}
        out = head(x, torch.from_numpy(data["onehots"]).to(dtype), zs)
        assert list(out) == list(factors)
        sum((out[k] * torch.from_numpy(data["w." + k]).to(dtype)).sum() for k in factors).backward()
        res = {"out." + k: v.detach().numpy() for k, v in out.items()}
        res["grad.pt_feat"] = x.grad.numpy()
        res.update({"grad." + name: p.grad.numpy() for name, p in head.named_parameters()})
        return res
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "models", "generator.py")):
        raise SystemExit("usage: make_attr_head_golden.py <reference root> (the directory that holds models/generator.py)")
    M = reference_module(sys.argv[1])
    rng = np.random.default_rng(20241020)
    blob = {}
    for case, (n_shared, layers, factors, n, instances, bare) in CASES.items():
        torch.manual_seed(7)
        head = M.GaussianAttrMLP(CLASSES, IN_DIM, Z_DIM, HIDDEN, n_shared, factors=dict(factors), n_layers=dict(layers))
        params = {name: p.detach().numpy().copy() for name, p in head.named_parameters()}
        for name in params:  # the initial values leave beta at its bias of 0 and the output layers small: move them
            if name.endswith("bias_beta") or name.startswith("fc_out_"):
                params[name] = params[name] + rng.normal(size=params[name].shape).astype(np.float32) * 0.3
        if "scale" in factors:
            params["fc_out_scale.weight"] = params["fc_out_scale.weight"] * 3.0
        ids = rng.integers(0, instances, size=n)
        ids[rng.choice(n, size=bare, replace=False)] = -1
        assert all((ids == g).any() for g in range(instances))
        data = {"pt_feat": rng.normal(size=(1, n, IN_DIM)).astype(np.float32),
                "onehots": np.eye(CLASSES, dtype=np.float32)[rng.integers(0, CLASSES, size=n)][None],
                "ids": ids.astype(np.int64), "z": rng.normal(size=(instances, Z_DIM)).astype(np.float32)}
        for k in factors:
            data["w." + k] = rng.normal(size=(1, n, 1 if k == "opacity" else 3)).astype(np.float32)
        r64, r32 = run(M, torch.float64, case, data, params), run(M, torch.float32, case, data, params)
        if "scale" in factors:  # the clamp must be active on some covered rows and inactive on others
            raw = (r64["out.scale"][0][ids >= 0] - 1.0) / factors["scale"]
            clamped = np.isclose(np.abs(raw), 1.0, rtol=0, atol=1e-12)
            assert clamped.any() and (~clamped).any(), (int(clamped.sum()), clamped.size)
            print(case, "scale: %d of %d values clamped" % (int(clamped.sum()), clamped.size))
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
            print(case, name, "float32 run: %.2e of the maximum" % err)
        assert all(not r64["out." + k][0][ids < 0].any() for k in factors)
    path = os.path.join(ROOT, "tests", "golden", "attr_head.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes,", len(blob), "arrays")


if __name__ == "__main__":
    main()
