"""Generates tests/golden/model_inputs.npz by running the REFERENCE's own Python on the CPU for the lines between the
visible point set and the rasterizer (scripts/inference.py:239-256): _get_pt_indexes_by_models, _get_pt_attrs_by_models
(with _get_z, utils.helpers.get_one_hot and get_projection_uv inside) and utils.helpers.get_gaussian_points.

  python tests/golden/make_model_inputs_golden.py <path of a GaussianCity checkout>

Run where a checkout of the reference exists; the fixture is data (inputs and recorded results), the reference sources
stay where they are.  Modules the reference imports at module level and these lines never touch are stubbed: cv2, plyfile,
open3d, lxml, torchvision.transforms, easydict, addict, tqdm, the CUDA extensions, spconv, torch_scatter, flash_attn.

The "models" are recorder callables: each keeps the seven arguments _get_gaussian_attributes hands a generator and returns
seeded attributes.  Cases (a few hundred rows each): both datasets' class tables; BLDG / CAR models present and absent; a
REST model that is None (its rows are dropped); a top-left point (tlp) present and absent; a PROJ_SIZE that is not a power
of two; a style LUT that lacks visible instances in the middle of the order, one that covers none of a model's instances
(zs None), and attribute dicts with and without the optional keys.
"""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
STUBS = ("cv2", "plyfile", "open3d", "lxml", "torchvision", "easydict", "addict", "tqdm", "spconv", "torch_scatter",
         "flash_attn", "footprint_extruder", "diff_gaussian_rasterization_ext", "grid_encoder_ext", "voxlib_ext", "extensions")


class _Any:
    """Stands for whatever a stubbed module is asked for: callable, subclassable, and every attribute is one again."""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Any()

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Any()


class _StubModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Any


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in STUBS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        return _StubModule(spec.name)

    def exec_module(self, module):
        module.__path__ = []


class Recorder:
    """A generator stand-in: keeps (proj_uv, rel_xyz, batch_idx, onehots, zs, proj_hf, proj_seg), returns seeded attributes."""

    def __init__(self, seed, keys):
        self.gen, self.keys, self.calls = torch.Generator().manual_seed(seed), keys, []

    def __call__(self, proj_uv, rel_xyz, batch_idx, onehots, zs, proj_hf, proj_seg):
        self.calls.append((proj_uv, rel_xyz, batch_idx, onehots, zs, proj_hf, proj_seg))
        n = proj_uv.size(1)
        width = {"rgb": 3, "xyz": 3, "scale": 3, "opacity": 1}
        self.out = {k: torch.rand(1, n, width[k], generator=self.gen) * 2 - 0.5 for k in self.keys}
        return self.out


def make_frame(inf, rng, dataset, instance_ids, n_rows):
    """A visible set as render() holds it after :237: pts [1,M,8], batch_idx [1,M,1], instances, classes, scales."""
    ids = np.sort(np.array(instance_ids, np.int16))
    ins = ids[rng.integers(0, len(ids), n_rows)]
    ins[0], ins[-1] = ids[0], ids[-1]
    ins[1:len(ids) + 1] = ids                              # every id at least once
    pts = np.empty((n_rows, 8), np.float32)
    pts[:, :3] = rng.integers(0, 2048, (n_rows, 3))
    pts[:, 3] = rng.integers(1, 5, n_rows)
    pts[:, 4] = ins
    pts[:, 5:] = rng.uniform(-1, 1, (n_rows, 3)).astype(np.float32)
    batch_idx = np.searchsorted(ids, ins).astype(np.int32)[:, None]
    pts_t, batch_t = torch.from_numpy(pts[None]), torch.from_numpy(batch_idx[None])
    instances = pts_t[:, :, [4]]
    classes = inf._instances_to_classes(dataset, instances)
    scales = inf.utils.helpers.get_point_scales(pts_t[:, :, [3]] * inf.CONSTANTS[dataset]["POINT_SCALE_FACTOR"], classes,
                                                inf.CONSTANTS[dataset]["SPECIAL_Z_SCALE_CLASSES"].values())
    return ids, pts_t, batch_t, instances, classes, scales


def run_case(inf, out, name, dataset, ids, n_rows, present, lut_ids, tlp, proj_size, keys, seed):
    rng = np.random.default_rng(seed)
    ids, pts, batch_idx, instances, classes, scales = make_frame(inf, rng, dataset, ids, n_rows)
    z_dim = 8
    gen = torch.Generator().manual_seed(seed)
    style_lut = {int(i): torch.rand(1, z_dim, generator=gen) for i in lut_ids}
    models = {k: (Recorder(seed * 10 + j, keys) if present[k] else None) for j, k in enumerate(("BLDG", "CAR", "REST"))}
    inf.CONSTANTS[dataset]["PROJ_SIZE"] = proj_size
    proj_tlp = None if tlp is None else torch.from_numpy(np.array(tlp)[None, ...])
    proj_hf, proj_seg = torch.zeros(1, 1, 4, 4), torch.zeros(1, 8, 4, 4)
    bldg_idx, car_idx, rest_idx = inf._get_pt_indexes_by_models(dataset, classes, models["BLDG"], models["CAR"])
    indexes = {"BLDG": bldg_idx, "CAR": car_idx, "REST": rest_idx}
    abs_xyz, cat_scales, pt_attrs = inf._get_pt_attrs_by_models(
        dataset, batch_idx, pts, scales, classes, instances, style_lut,
        {"TD_HF": proj_hf, "SEG": proj_seg, "TLP": proj_tlp}, indexes, models)
    p = name + "/"
    out[p + "dataset"] = np.array(dataset)
    out[p + "pts"], out[p + "batch_idx"] = pts.numpy(), batch_idx.numpy()
    out[p + "instances"], out[p + "classes"], out[p + "scales"] = ids, classes.numpy(), scales.numpy()
    out[p + "present"] = np.array([present[k] for k in ("BLDG", "CAR", "REST")])
    out[p + "lut_ids"] = np.array(sorted(style_lut), np.int32)
    out[p + "lut_codes"] = (torch.cat([style_lut[i] for i in sorted(style_lut)]).numpy() if style_lut
                            else np.zeros((0, z_dim), np.float32))
    out[p + "tlp"] = np.zeros(0, np.int64) if tlp is None else np.array(tlp)
    out[p + "proj_size"] = np.array(proj_size)
    out[p + "keys"] = np.array(sorted(keys))
    for k, model in models.items():
        out[p + k + "/mask"] = indexes[k].numpy().astype(bool)
        called = model is not None and len(model.calls) == 1
        out[p + k + "/called"] = np.array(called)
        if not called:
            assert model is None or not model.calls
            continue
        proj_uv, rel_xyz, b_idx, onehots, zs, hf, seg = model.calls[0]
        assert hf is proj_hf and seg is proj_seg
        out[p + k + "/proj_uv"], out[p + k + "/rel_xyz"] = proj_uv.numpy(), rel_xyz.numpy()
        out[p + k + "/batch_idx"], out[p + k + "/onehots"] = b_idx.numpy(), onehots.numpy()
        out[p + k + "/zs_is_none"] = np.array(zs is None)
        if zs is not None:
            out[p + k + "/zs_keys"] = np.array(list(zs.keys()), np.int32)       # dict order
            out[p + k + "/zs_z"] = torch.cat([v["z"] for v in zs.values()]).numpy()
            out[p + k + "/zs_idx"] = torch.cat([v["idx"] for v in zs.values()]).numpy()
        for a, v in model.out.items():
            out[p + k + "/attr_" + a] = v.numpy()
    out[p + "abs_xyz"], out[p + "cat_scales"] = abs_xyz.numpy().copy(), cat_scales.numpy().copy()
    for a, v in pt_attrs.items():
        out[p + "cat_" + a] = v.numpy()
    out[p + "gs_pts"] = inf.utils.helpers.get_gaussian_points(abs_xyz, cat_scales, pt_attrs).numpy()   # (shifts abs_xyz in place)


def main(ref):
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, ref)
    import scripts.inference as inf                 # the reference's own lines
    all_keys, ge, ki = ("rgb", "xyz", "scale", "opacity"), "GOOGLE_EARTH", "KITTI_360"
    ge_ids = [1, 3, 5, 6, 100, 101, 102, 105, 230, 231, 1001]
    ki_ids = [1, 4, 5, 6, 100, 101, 340, 341, 9999, 10000, 10003, 10010]
    out = {}
    run_case(inf, out, "ge_all", ge, ge_ids, 300, dict(BLDG=True, CAR=False, REST=True), [3, 100, 102, 105, 231, 777], None, 2048,
             all_keys, 1)
    run_case(inf, out, "ge_tlp", ge, ge_ids, 257, dict(BLDG=True, CAR=True, REST=True), [101, 230], [37, 1205], 2048, ("rgb",), 2)
    run_case(inf, out, "ge_no_bldg", ge, ge_ids, 200, dict(BLDG=False, CAR=False, REST=True), [1, 5, 100, 101], None, 1000,
             ("rgb", "scale"), 3)
    run_case(inf, out, "ki_all", ki, ki_ids, 320, dict(BLDG=True, CAR=True, REST=True), [100, 341, 10003, 10010, 4], [-12, 640],
             2048, all_keys, 4)
    run_case(inf, out, "ki_no_car", ki, ki_ids, 190, dict(BLDG=True, CAR=False, REST=True), [10000, 9999], [5, 5], 1280,
             ("rgb", "opacity"), 5)
    run_case(inf, out, "ki_no_rest", ki, ki_ids, 150, dict(BLDG=True, CAR=True, REST=False), [1, 4, 5, 6], None, 2048,
             ("rgb", "xyz"), 6)                     # the LUT covers no building and no car: zs None for both
    path = os.path.join(HERE, "model_inputs.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
