"""Generates tests/golden/train_inputs.npz by running the REFERENCE's own Python on the CPU for the lines between the data
loader and the generator (core/train.py:207-224): NormalizePointCords and ToTensor for the rows, then the slices,
instances_to_classes, utils.helpers.get_point_scales, get_one_hot, get_z and get_projection_uv.

  python tests/golden/make_train_inputs_golden.py <path of a GaussianCity checkout>

Run where a checkout of the reference exists; the fixture is data (inputs, recorded results, the CPU generator's state
before and after, and the values of config.py these lines read), the reference sources stay where they are.  Modules the
reference imports at module level and these lines never touch are stubbed: cv2, plyfile, tqdm.  easydict need not be installed
either: config.py gets a dict with attribute access under that name, so its own assignments run.  instances_to_classes is
a method of the dataset classes, whose constructors list files: it is called unbound on a stand-in `self` that carries cfg.

Cases: both datasets' rules, 300 rows with about 12 distinct ids (building ids at both ends of BLDG_RANGE in both
parities, every special z class, KITTI-360's car range at both ends), z_dim 256, 8 and None; proj_tlp None and int64 [1,2].
"""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
STUBS = ("cv2", "plyfile", "tqdm")
CFG_KEYS = ("BLDG_RANGE", "BLDG_FACADE_CLSID", "BLDG_ROOF_CLSID", "CAR_RANGE", "CAR_CLSID", "N_CLASSES", "PROJ_SIZE")
SEED = 2024


class _Any:
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


class AttrDict(dict):
    """What config.py needs of EasyDict: keys as attributes."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def __setattr__(self, name, value):
        self[name] = value


def make_rows(transforms, rng, ids, n_rows):
    """pts [1,N,9] as the loader hands it over: five columns (x, y, z, scale, instance) through NormalizePointCords and
    ToTensor."""
    ids = np.sort(np.array(ids, np.int64))
    ins = ids[rng.integers(0, len(ids), n_rows)]
    ins[:len(ids)] = ids[rng.permutation(len(ids))]        # every id at least once, in no order
    pts = np.empty((n_rows, 5), np.int16)
    pts[:, :3] = rng.integers(0, 2048, (n_rows, 3))
    pts[:, 3] = rng.integers(1, 5, n_rows)
    pts[:, 4] = ins
    centers = {int(i): (float(rng.integers(0, 2048)), float(rng.integers(0, 2048)), float(rng.integers(0, 90)),
                        float(rng.integers(1, 90)), float(rng.integers(1, 400))) for i in ids}
    data = transforms.NormalizePointCords(None, ["pts"])({"pts": pts, "centers": centers})
    data = transforms.ToTensor(None, ["pts"])(data)
    return data["pts"].unsqueeze(0)


def run_case(out, name, helpers, dataset, cfg, dataset_name, pts, z_dim, tlp, scale_factor):
    node = cfg.DATASETS[dataset_name]
    proj_tlp = None if tlp is None else torch.from_numpy(np.array(tlp, np.int64)[None, ...])
    torch.manual_seed(SEED)
    before = torch.get_rng_state()
    # core/train.py:207-224
    abs_xyz = pts[:, :, :3]
    bch_idx = pts[:, :, 8].long()
    instances = pts[:, :, [4]]
    classes = dataset.instances_to_classes(types.SimpleNamespace(cfg=cfg), instances)
    scales = pts[:, :, [3]] * scale_factor
    scales = helpers.get_point_scales(scales, classes, list(node.Z_SCALE_SPECIAL_CLASSES.values()))
    onehots = helpers.get_one_hot(classes, node.N_CLASSES)
    z = helpers.get_z(instances, z_dim)
    proj_uv = helpers.get_projection_uv(abs_xyz, proj_tlp, node.PROJ_SIZE)
    after = torch.get_rng_state()
    p = name + "/"
    out[p + "dataset"], out[p + "z_dim"] = np.array(dataset_name), np.array(-1 if z_dim is None else z_dim)
    out[p + "tlp"] = np.zeros((0, 2), np.int64) if tlp is None else proj_tlp.numpy()
    out[p + "bch_idx"], out[p + "classes"], out[p + "scales"] = bch_idx.numpy(), classes.numpy(), scales.numpy()
    out[p + "onehots"], out[p + "proj_uv"] = onehots.numpy(), proj_uv.numpy()
    if z is None:
        assert torch.equal(before, after)
    else:
        out[p + "z_keys"] = np.array(list(z.keys()), np.int32)                 # dict order
        out[p + "z_codes"] = torch.cat([v["z"] for v in z.values()]).numpy()
        out[p + "z_idx"] = np.packbits(torch.cat([v["idx"] for v in z.values()]).numpy(), axis=1)
        out[p + "rng_after"] = after.numpy()
    return before


def main(ref):
    sys.meta_path.insert(0, _StubFinder())
    easydict = types.ModuleType("easydict")
    easydict.EasyDict = AttrDict
    sys.modules["easydict"] = easydict
    sys.path.insert(0, ref)
    import utils.datasets as datasets          # the reference's own lines
    import utils.helpers as helpers
    import utils.transforms as transforms
    from config import cfg
    scale_factor = cfg.NETWORK.GAUSSIAN.SCALE_FACTOR
    out = {"scale_factor": np.array(scale_factor, np.float64), "seed": np.array(SEED)}
    classes = {"GOOGLE_EARTH": datasets.GoogleDataset, "KITTI_360": datasets.Kitti360Dataset}
    ids = {"GOOGLE_EARTH": [1, 3, 5, 6, 100, 101, 230, 1001, 4444, 32766, 32767],
           "KITTI_360": [0, 1, 4, 5, 6, 100, 101, 9998, 9999, 10000, 10003, 16383]}
    for k, (dataset_name, cls) in enumerate(classes.items()):
        node = cfg.DATASETS[dataset_name]
        for key in CFG_KEYS:
            if key in node:
                out["cfg/%s/%s" % (dataset_name, key)] = np.array(node[key])
        out["cfg/%s/Z_SCALE_SPECIAL_CLASSES" % dataset_name] = np.array(sorted(node.Z_SCALE_SPECIAL_CLASSES.values()))
        short = "ge" if dataset_name == "GOOGLE_EARTH" else "ki"
        pts = make_rows(transforms, np.random.default_rng(7 + k), ids[dataset_name], 300)
        out[short + "/pts"] = pts.numpy()
        for z_dim, tlp in ((256, None), (8, [37 + k, 1205]), (None, [-12, 640]) if k else (None, None)):
            name = "%s/z%s" % (short, "none" if z_dim is None else z_dim)
            before = run_case(out, name, helpers, cls, cfg, dataset_name, pts, z_dim, tlp, scale_factor)
    out["rng_before"] = before.numpy()         # torch.manual_seed(SEED): the same for every case
    path = os.path.join(HERE, "train_inputs.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
