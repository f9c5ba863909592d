#!/usr/bin/env python
"""Generates tests/golden/attr_chain.npz with the REFERENCE's own models/generator.py, imported on the CPU: its
GaussianAttrMLP under no_grad, without style codes (the background generator: z_dim None, zs None) and with them (the
building generator), twice per case on the same seeded parameters and inputs, once in float64 (the target) and once in
float32 (the reference's own error).  Run in the build container only (the reference does not exist on the GPU box):

    python tests/golden/make_attr_chain_golden.py <reference root>

generator.py is loaded by path; empty modules stand in for its two imports that the head does not use
(`extensions.grid_encoder`, `models.pt_v3`).  The fixture holds inputs, parameters and the reference's outputs -- data
only.  Per case <c>:

    <c>.z_dim, <c>.layers, <c>.factors      z_dim (-1: None); n_layers and factors of xyz, rgb, scale, opacity (-1: the key
                                            is absent); n_shared_layers is 1 in every case
    <c>.pt_feat, <c>.onehots                float32 inputs [b, n, 24] and [b, n, 7]
    <c>.ids, <c>.z                          (with codes) int64 [n]: the row's instance in dict order, -1 without a style;
                                            float32 codes [instances, 16]
    <c>.param.<name>                        float32 parameters
    <c>.out.<key>                           float64 results
    <c>.err32.out.<key>                     max|x32 - x64| / max|x64| of the reference's float32 run

Cases: bg -- zs None, one rgb layer.  bg2 -- zs None, two rgb layers and one opacity layer, batch 2: upstream applies
every layer of a key to f and keeps the last, and the maker asserts that the result is further from the two layers applied
one after the other than the float32 error, so the case tells the two apart.  bldg -- three instances, five rows without a
style, one layer per key, scale's clamp active on some rows and not on others.
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
# z_dim, n_layers and factors per key, batch, rows, instances, rows without a style
CASES = {
    "bg": (None, {"rgb": 1}, {"rgb": 2.0}, 1, 200, 0, 0),
    "bg2": (None, {"rgb": 2, "opacity": 1}, {"rgb": 2.0, "opacity": 0.6}, 2, 100, 0, 0),
    "bldg": (Z_DIM, {"xyz": 1, "rgb": 1, "scale": 1, "opacity": 1}, {"xyz": 0.75, "rgb": 2.0, "scale": 0.5, "opacity": 0.6}, 1, 203,
             3, 5),
}


def reference_module(ref_root):
    for name in ("extensions", "extensions.grid_encoder", "models", "models.pt_v3"):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location("reference_generator", os.path.join(ref_root, "models", "generator.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def build(M, dtype, case, params):
    z_dim, layers, factors = CASES[case][:3]
    head = M.GaussianAttrMLP(CLASSES, IN_DIM, z_dim, HIDDEN, 1, factors=dict(factors), n_layers=dict(layers)).to(dtype)
    with torch.no_grad():
        for name, value in params.items():
            head.get_parameter(name).copy_(torch.from_numpy(value).to(dtype))
    return head


def run(M, dtype, case, data, params):
    factors = CASES[case][2]
    torch.set_default_dtype(dtype)
    try:
        head = build(M, dtype, case, params)
        zs = None
        if "z" in data:
            ids = torch.from_numpy(data["ids"])
            zs = {100 + g: {"z": torch.from_numpy(data["z"][g:g + 1]).to(dtype), "idx": (ids == g).unsqueeze(0)}
                  for g in range(data["z"].shape[0])}
        with torch.no_grad():
            out = head(torch.from_numpy(data["pt_feat"]).to(dtype), torch.from_numpy(data["onehots"]).to(dtype), zs)
        assert list(out) == list(factors)
        return {"out." + k: v.numpy() for k, v in out.items()}
    finally:
        torch.set_default_dtype(torch.float32)


def rgb_layers_one_after_the_other(M, data, params):
    """bg2's rgb in float64 with fc_2_rgb_1 applied to fc_2_rgb_0's output: what upstream does NOT compute."""
    head = build(M, torch.float64, "bg2", params)
    with torch.no_grad():
        x, hot = torch.from_numpy(data["pt_feat"]).double(), torch.from_numpy(data["onehots"]).double()
        f = head.act(head.fc_1(x) + head.fc_m_a(hot))
        f = head.act(head.fc_2_rgb_1(head.act(head.fc_2_rgb_0(f))))
        return ((torch.sigmoid(head.fc_out_rgb(f)) - 0.5) * CASES["bg2"][2]["rgb"]).numpy()


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "models", "generator.py")):
        raise SystemExit("usage: make_attr_chain_golden.py <reference root> (the directory that holds models/generator.py)")
    M = reference_module(sys.argv[1])
    rng = np.random.default_rng(20261020)
    blob = {}
    for case, (z_dim, layers, factors, b, n, instances, bare) in CASES.items():
        torch.manual_seed(11)
        head = M.GaussianAttrMLP(CLASSES, IN_DIM, z_dim, HIDDEN, 1, factors=dict(factors), n_layers=dict(layers))
        params = {name: p.detach().numpy().copy() for name, p in head.named_parameters()}
        for name in params:  # the initial values leave beta at its bias of 0 and the output layers small: move them
            if name.endswith("bias_beta") or name.startswith("fc_out_"):
                params[name] = params[name] + rng.normal(size=params[name].shape).astype(np.float32) * 0.3
        if "scale" in factors:
            params["fc_out_scale.weight"] = params["fc_out_scale.weight"] * 3.0
        data = {"pt_feat": rng.normal(size=(b, n, IN_DIM)).astype(np.float32),
                "onehots": np.eye(CLASSES, dtype=np.float32)[rng.integers(0, CLASSES, size=(b, n))]}
        ids = None
        if instances:
            ids = rng.integers(0, instances, size=n)
            ids[rng.choice(n, size=bare, replace=False)] = -1
            assert all((ids == g).any() for g in range(instances)) and (ids < 0).sum() == bare
            data["ids"], data["z"] = ids.astype(np.int64), rng.normal(size=(instances, Z_DIM)).astype(np.float32)
        r64, r32 = run(M, torch.float64, case, data, params), run(M, torch.float32, case, data, params)
        if "scale" in factors:  # the clamp must be active on some covered rows and inactive on others
            raw = (r64["out.scale"][0][ids >= 0] - 1.0) / factors["scale"]
            clamped = np.isclose(np.abs(raw), 1.0, rtol=0, atol=1e-12)
            assert clamped.any() and (~clamped).any(), (int(clamped.sum()), clamped.size)
            print(case, "scale: %d of %d values clamped" % (int(clamped.sum()), clamped.size))
        blob["%s.z_dim" % case] = np.asarray(-1 if z_dim is None else z_dim, np.int64)
        blob["%s.layers" % case] = np.asarray([layers.get(k, -1) for k in KEYS], np.int64)
        blob["%s.factors" % case] = np.asarray([factors.get(k, -1.0) for k in KEYS], np.float64)
        blob.update({"%s.%s" % (case, k): v for k, v in data.items()})
        blob.update({"%s.param.%s" % (case, k): v for k, v in params.items()})
        worst = 0.0
        for name, x64 in r64.items():
            assert x64.dtype == np.float64 and r32[name].dtype == np.float32, (name, x64.dtype, r32[name].dtype)
            assert x64.shape == (b, n, 1 if name == "out.opacity" else 3), (name, x64.shape)
            err = float(np.abs(r32[name].astype(np.float64) - x64).max() / np.abs(x64).max())
            assert err > 0, name
            worst = max(worst, err)
            blob["%s.%s" % (case, name)] = x64
            blob["%s.err32.%s" % (case, name)] = np.asarray(err)
            print(case, name, "float32 run: %.2e of the maximum" % err)
        if ids is not None:
            assert all(not r64["out." + k][0][ids < 0].any() for k in factors)
        if case == "bg2":  # the last-layer rule: chaining the two rgb layers must land somewhere else
            other = rgb_layers_one_after_the_other(M, data, params)
            gap = float(np.abs(other - r64["out.rgb"]).max() / np.abs(r64["out.rgb"]).max())
            print(case, "rgb with its two layers chained: %.2e of the maximum away (largest err32 %.2e)" % (gap, worst))
            assert gap > worst, (gap, worst)
    path = os.path.join(ROOT, "tests", "golden", "attr_chain.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes,", len(blob), "arrays")


if __name__ == "__main__":
    main()
