"""The generator's inputs of a training step (include/gcv.h K23 / K24): what lies between the data loader and the generator
in core/train.py:207-224, on crops of N rows with I distinct building instances, KITTI-360's rule, a top-left point.

  torch   a torch-ops formulation of those lines on the device tensor, written from their behaviour: five slices; the
          three masks, the copy and the masked assignments of instances_to_classes; get_point_scales (ones_like, repeat,
          isin, a masked assignment); get_one_hot (zeros, scatter_); get_z -- torch.unique, one .item() per instance, per
          instance one torch.randn(1, z_dim), one host-to-device copy and one N-element compare; get_projection_uv;
  device  train_inputs.prepare.

Both sides run in one process, alternating, around blocks of calls that end in a synchronise; host wall time per call,
median over the blocks.  Results are compared bit for bit per shape, the codes from the same seed included.  Appends one
JSON line to --out.
    python tools/train_inputs_bench.py --out profiles/train_inputs.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussiancity_amd import train_inputs as TI  # noqa: E402

SHAPES = ((16384, 1), (16384, 16), (16384, 256), (262144, 256))
Z_DIMS = (None, 256)


def torch_inputs(pts, rule, z_dim, proj_tlp):
    """The host-driven path on the device tensor."""
    abs_xyz = pts[:, :, :3]
    rel_xyz = pts[:, :, 5:8]
    bch_idx = pts[:, :, 8].long()
    instances = pts[:, :, [4]]
    in_bldg = (instances >= rule.bldg_ins_min) & (instances < rule.bldg_ins_max)
    facade = in_bldg & (instances % 2 == 0)
    roof = (instances >= rule.bldg_ins_min) & (instances < rule.bldg_ins_max) & (instances % 2 == 1)
    car = (instances >= rule.car_ins_min) & (instances < rule.car_ins_max)
    classes = instances.clone()
    classes[facade] = rule.facade_class
    classes[roof] = rule.roof_class
    classes[car] = rule.car_class
    scales = pts[:, :, [3]] * rule.scale_factor
    scales = torch.ones_like(scales).repeat(1, 1, 3) * scales
    scales[..., 2][torch.isin(classes.squeeze(dim=-1), torch.tensor(list(rule.special_z_classes), device=classes.device))] = 1
    onehots = torch.zeros(pts.size(0), pts.size(1), rule.n_classes).to(classes.device)
    onehots.scatter_(2, classes.long(), 1)
    z = None
    if z_dim is not None:
        ids = [i.item() for i in torch.unique(instances).short()]
        codes = {ui: torch.randn(1, z_dim).to(instances.device) for ui in ids}
        z = {ui: {"z": codes[ui], "idx": instances[..., 0] == ui} for ui in ids}
    uv = abs_xyz[..., :2] - proj_tlp.unsqueeze(dim=1)
    uv[..., 0] /= rule.proj_size
    uv[..., 1] /= rule.proj_size
    return abs_xyz, rel_xyz, bch_idx, instances, classes, scales, onehots, z, uv * 2 - 1


def make_pts(n, n_ins, dev):
    gen = torch.Generator().manual_seed(n + n_ins)
    ids = (torch.randperm(9900, generator=gen)[:n_ins] + 100).sort().values.float()
    ins = ids[torch.randint(0, n_ins, (n,), generator=gen)]
    ins[:n_ins] = ids
    pts = torch.empty(1, n, 9)
    pts[0, :, :3] = torch.rand(n, 3, generator=gen) * 2048
    pts[0, :, 3] = torch.rand(n, generator=gen) * 4 + 0.5
    pts[0, :, 4] = ins
    pts[0, :, 5:8] = torch.rand(n, 3, generator=gen) * 2 - 1
    pts[0, :, 8] = torch.searchsorted(ids, ins).float()
    return pts.to(dev)


def same(a, b):
    eq = lambda x, y: x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)  # noqa: E731
    ok = all(eq(x, getattr(b, k)) for x, k in zip(a[:7], ("abs_xyz", "rel_xyz", "bch_idx", "instances", "classes", "scales", "onehots")))
    ok = ok and eq(a[8], b.proj_uv) and (a[7] is None) == (b.z is None)
    if a[7] is not None:
        ok = ok and list(a[7]) == list(b.z)
        ok = ok and eq(torch.cat([v["z"] for v in a[7].values()]), b.z.codes)
        ok = ok and all(torch.equal(v["idx"][0], b.z.group == g) for g, v in enumerate(a[7].values()))
    return bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=8, help="calls per block")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_inputs.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_inputs_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    rule = TI.RULE_KITTI_360()
    tlp = torch.tensor([[37, 1205]], device=dev)
    ws = TI.Workspace(dev)
    result, equal = {}, True
    for n, n_ins in SHAPES:
        pts = make_pts(n, n_ins, dev)
        for z_dim in Z_DIMS:
            sides = {"torch": lambda: torch_inputs(pts, rule, z_dim, tlp),
                     "device": lambda: TI.prepare(pts, rule, z_dim, tlp, workspace=ws)}
            torch.manual_seed(1)
            a = sides["torch"]()
            torch.manual_seed(1)
            b = sides["device"]()
            equal = same(a, b) and int(b.flag) == 0 and equal
            del a, b

            def block(side):
                for _ in range(args.calls):
                    out = sides[side]()
                torch.cuda.synchronize()
                return out

            for side in sides:
                block(side)
                block(side)                                       # allocator pools, code objects and clocks up
            wall = {"torch": [], "device": []}
            for _ in range(args.blocks):
                for side in sides:                                # alternating
                    t0 = time.perf_counter()
                    block(side)
                    wall[side].append(1e3 * (time.perf_counter() - t0) / args.calls)
            t_ms, d_ms = statistics.median(wall["torch"]), statistics.median(wall["device"])
            result["n%d_i%d_z%s" % (n, n_ins, z_dim)] = {
                "rows": n, "instances": n_ins, "z_dim": z_dim, "torch_ms_per_call": round(t_ms, 4),
                "device_ms_per_call": round(d_ms, 4), "torch_over_device": round(t_ms / d_ms, 2),
                "torch_ms_blocks": [round(v, 4) for v in wall["torch"]], "device_ms_blocks": [round(v, 4) for v in wall["device"]]}
    rec = {"tool": "tools/train_inputs_bench.py", "device": torch.cuda.get_device_name(0),
           "shape": {"rule": "KITTI_360", "proj_tlp": "int64 [1,2] on the device", "pts": "[1, rows, 9] float32"},
           "timing": "host wall time per call around blocks of %d calls ending in a synchronise; both sides in one process, "
                     "alternating; median of %d blocks; the codes are drawn on the host on both sides" % (args.calls, args.blocks),
           "per_shape": result, "device_equals_torch_bit_for_bit_on_every_shape": equal}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))
    if not equal:
        raise SystemExit("device and torch results differ")


if __name__ == "__main__":
    main()
