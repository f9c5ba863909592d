"""Per-model generator inputs and [N,14] assembly (include/gcv.h K17 / K18) on the frame of tools/visible_set_bench.py: the
2048 x 2048 synthetic layout (gcity-layout-v1, seed 2001), a 960 x 540 image, the 24-pose orbit, its box table.  Per pose
the visible set comes from points.visible_point_set; the timed part is what lies between it and the rasterizer, without
any generator (the attribute tensors are made beforehand, per pose and model):

  torch   a torch-ops formulation of scripts/inference.py:239-256 on the device tensors, written from its behaviour: three
          isin masks; per model the empty test (a host wait), five boolean-mask gathers, torch.unique and the Python
          renumbering loop; per visible instance one .item(), one host-to-device copy of its code and one M-element mask;
          the one-hots, the projection uv, the per-key torch.cat and helpers.get_gaussian_points;
  device  model_inputs.split_by_model + model_inputs.gaussian_points14.

Both sides run in one process, alternating, around blocks of poses that end in a synchronise; host wall time per frame,
median over the blocks, per pose count.  Results are compared bit for bit on every pose.  GOOGLE_EARTH's layout only: two
models (BLDG, REST); KITTI-360's three-model frames are not measured.  Appends one JSON line to --out.
    python tools/model_inputs_bench.py --out profiles/model_inputs.jsonl
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gaussiancity_amd import helpers as H  # noqa: E402
from gaussiancity_amd import model_inputs as MI  # noqa: E402
from gaussiancity_amd import points as P  # noqa: E402
from gaussiancity_amd import synth  # noqa: E402
from visible_set_bench import boxes_table  # noqa: E402

N_CLASSES, PROJ_SIZE, Z_DIM = 8, 2048, 256
BLDG_CLASSES = (P.CLASS_RULE_GOOGLE_EARTH.facade_class, P.CLASS_RULE_GOOGLE_EARTH.roof_class)


def torch_split(vs, lut):
    """The host-driven path on device tensors: {model: the generator's arguments}, and the concatenated xyz and scales."""
    pts, batch_idx, classes, scales = vs.pts, vs.batch_idx, vs.classes, vs.scales
    instances = pts[:, :, [4]]
    flat = classes.squeeze()
    bldg = torch.isin(flat, torch.tensor(BLDG_CLASSES, device=flat.device))
    car = torch.zeros_like(flat)                            # GOOGLE_EARTH has no CAR class
    masks = {"BLDG": bldg, "CAR": car, "REST": ~torch.logical_or(bldg, car)}
    per, xyz, sc = {}, [], []
    for name, idx in masks.items():
        if torch.sum(idx) == 0:
            continue
        idx = idx.bool()
        b = batch_idx[:, idx].clone()
        for i, bi in enumerate(torch.unique(b)):
            b[b == bi] = i
        p, c, ins = pts[:, idx], classes[:, idx], instances[:, idx]
        ids = [v.item() for v in torch.unique(ins).short()]
        codes = {ui: lut[ui].to(ins.device) for ui in ids if ui in lut}
        zs = {ui: {"z": codes[ui], "idx": ins[..., 0] == ui} for ui in ids if ui in codes} if codes else None
        onehots = torch.zeros(1, p.size(1), N_CLASSES).to(p.device)
        onehots.scatter_(2, c.long(), 1)
        uv = p[..., :2].clone()
        uv[..., 0] /= PROJ_SIZE
        uv[..., 1] /= PROJ_SIZE
        per[name] = {"proj_uv": uv * 2 - 1, "rel_xyz": p[:, :, 5:8], "batch_idx": b[..., 0], "onehots": onehots, "zs": zs}
        xyz.append(p[:, :, :3])
        sc.append(scales[:, idx])
    return per, torch.cat(xyz, dim=1), torch.cat(sc, dim=1)


def torch_frame(vs, lut, attrs):
    per, xyz, sc = torch_split(vs, lut)
    cat = {k: torch.cat([attrs[name][k] for name in per], dim=1) for k in next(iter(attrs.values()))}
    return per, H.get_gaussian_points(xyz, sc, cat)


def device_frame(vs, rule, table, attrs, ws):
    split = MI.split_by_model(vs, rule, table, None, PROJ_SIZE, workspace=ws)
    return split, MI.gaussian_points14(split, attrs)


def same(per, gs_t, split, gs_d):
    ok = torch.equal(gs_t.view(torch.int32), gs_d.view(torch.int32)) and list(per) == list(split.models)
    for name, a in per.items():
        m = split.models[name]
        ok = ok and all(torch.equal(a[k].view(torch.int32), getattr(m, k).view(torch.int32)) for k in ("proj_uv", "rel_xyz", "onehots"))
        ok = ok and torch.equal(a["batch_idx"], m.batch_idx) and (a["zs"] is None) == (m.zs is None)
        if a["zs"] is not None:
            ok = ok and list(a["zs"]) == list(m.zs)
            ok = ok and all(torch.equal(v["idx"], w["idx"]) and torch.equal(v["z"].view(torch.int32), w["z"].view(torch.int32))
                            for v, w in zip(a["zs"].values(), m.zs.values()))
    return bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout-size", type=int, default=2048)
    ap.add_argument("--poses", default="24,8,1", help="pose counts per block, the first is the orbit's length")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_inputs.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("model_inputs_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    counts = [int(v) for v in args.poses.split(",")]
    size, Wimg, Himg = args.layout_size, 960, 540
    L = synth.s_layout(size, 2001)
    inv = {v: k for k, v in synth.LAYOUT_CLASSES.items()}
    maps = [torch.from_numpy(L[k]).to(dev) for k in ("INS", "TD_HF", "BU_HF", "PTS")]
    rig = synth.layout_camera(size, Wimg, Himg)[0]
    rows = P.extrude_points(True, inv, synth.LAYOUT_SCALES, synth.LAYOUT_SEG_INS, *maps)
    table = boxes_table(rows)
    vol_ws, sets = P.VolumeWorkspace(dev), []
    for i in range(max(counts)):
        cam_pos, cam_quat = synth.layout_camera(size, Wimg, Himg, pose=i)[1:]
        vp = P.visible_point_map(rows, rig, cam_pos, cam_quat, 0, workspace=vol_ws)[0]
        sets.append(P.visible_point_set(rows, vp, table, P.CLASS_RULE_GOOGLE_EARTH))
    del vol_ws, maps
    # a style LUT as get_style_lut leaves it for a building generator with codes and a background generator without:
    # host tensors for the building instances, every seventh missing
    known = torch.nonzero(~torch.isnan(table[:, 0])).reshape(-1).tolist()
    gen = torch.Generator().manual_seed(3)
    lut = {i: torch.rand(1, Z_DIM, generator=gen) for n, i in enumerate(known) if i >= 100 and n % 7}
    style = MI.style_table(lut, dev)
    rule, ws = MI.MODEL_RULE_GOOGLE_EARTH(), P.VisibleSetWorkspace(dev)
    attrs, shape = [], []
    for vs in sets:                                           # the generators' outputs, made beforehand
        split = MI.split_by_model(vs, rule, style, workspace=ws)
        attrs.append({name: {k: torch.rand((1, m.index.shape[0], w), device=dev) for k, w in (("rgb", 3), ("xyz", 3), ("scale", 3), ("opacity", 1))}
                      for name, m in split.models.items()})
        shape.append((int(vs.pts.shape[1]), int(vs.instances.numel()), split.counts["BLDG"][2], len(split.models)))
    equal = all(same(*torch_frame(vs, lut, a), *device_frame(vs, rule, style, a, ws)) for vs, a in zip(sets, attrs))

    def block(side, n):
        for vs, a in zip(sets[:n], attrs[:n]):
            out = torch_frame(vs, lut, a) if side == "torch" else device_frame(vs, rule, style, a, ws)
        torch.cuda.synchronize()
        return out

    result = {}
    for n in counts:
        for side in ("torch", "device"):
            block(side, n)
            block(side, n)                                    # allocator pools, code objects and clocks up
        wall = {"torch": [], "device": []}
        for _ in range(args.blocks):
            for side in ("torch", "device"):                  # alternating
                t0 = time.perf_counter()
                block(side, n)
                wall[side].append(1e3 * (time.perf_counter() - t0) / n)
        t_ms, d_ms = statistics.median(wall["torch"]), statistics.median(wall["device"])
        result[str(n)] = {"torch_ms_per_frame": round(t_ms, 4), "device_ms_per_frame": round(d_ms, 4),
                          "torch_over_device": round(t_ms / d_ms, 2),
                          "torch_ms_blocks": [round(v, 4) for v in wall["torch"]],
                          "device_ms_blocks": [round(v, 4) for v in wall["device"]]}
    rec = {"tool": "tools/model_inputs_bench.py", "device": torch.cuda.get_device_name(0),
           "shape": {"layout": [size, size], "image": [Wimg, Himg], "n_points": int(rows.shape[0]), "z_dim": Z_DIM,
                     "style_codes": len(lut), "dataset_rule": "GOOGLE_EARTH (BLDG + REST; no CAR model)",
                     "min_max_over_poses": {k: [min(v[i] for v in shape), max(v[i] for v in shape)] for i, k in enumerate(
                         ("visible_points", "instances", "instances_with_a_code", "models_with_rows"))}},
           "timing": "host wall time per frame around blocks of the first n poses ending in a synchronise; both sides in one "
                     "process, alternating; median of %d blocks; no generator in either side" % args.blocks,
           "per_pose_count": result, "device_equals_torch_bit_for_bit_on_every_pose": equal}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))
    if not equal:
        raise SystemExit("device and torch results differ")


if __name__ == "__main__":
    main()
