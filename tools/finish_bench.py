"""Frame finish (include/gcv.h K19, gaussiancity_amd/finish.py) against the torch-ops form of scripts/inference.py:255,
264-272 and :665 on the device, at 960 x 540 and 1408 x 376, with 0 %, 30 % and 100 % of the pixels showing a road, for
the float frame and for the uint8 frame:

  torch   reflect pad + depthwise conv2d with the same weights (what GaussianBlur runs); the mask
          (ins_map == ROAD).repeat(1, 3, 1, 1).float() from an ins_map already on the device ("torch") and from a numpy
          ins_map as upstream has it ("torch_numpy_map": one more host-to-device copy); blur * mask + img * (1 - mask);
          for the uint8 frame InferenceLoop.to_uint8_hwc on top;
  device  finish.road_blur: one launch.

Both sides run in one process on the same stream, alternating, around blocks of calls that end in a synchronise; host
wall time per call, median over the blocks.  Launches per frame are counted with torch.profiler in a pass of their own
after the timing.  Results are compared on every case: non-road pixels bit for bit, road pixels within the float32
summation bound of each other, bytes within 1.

Second part: what the step adds to the frame of bench.py --inference-loop (518 400 points, 960 x 540, the 24-pose orbit,
frames.InferenceLoop): the loop with to_uint8_hwc on the float image, the same loop finished through finish_fn
(30 % road), and the loop whose blend kernel stores the bytes (no blur possible).  Appends one JSON line to --out.
    python tools/finish_bench.py --out profiles/frame_finish.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussiancity_amd import finish  # noqa: E402
from gaussiancity_amd import synth  # noqa: E402
from gaussiancity_amd.frames import InferenceLoop  # noqa: E402

ROAD = synth.LAYOUT_CLASSES["ROAD"]


def torch_finish(img, ins_map, w33, as_uint8):
    """The upstream lines on the device.  img [3,H,W]; ins_map int16 [H,W] on the device, or numpy."""
    if isinstance(ins_map, np.ndarray):
        ins_map = torch.from_numpy(ins_map).to(img.device)
    x = img[None]
    k = w33.shape[-1]
    blurred = F.conv2d(F.pad(x, (k // 2,) * 4, mode="reflect"), w33, groups=3)
    road_mask = (ins_map[None, None] == ROAD).repeat(1, 3, 1, 1).float()
    out = (blurred * road_mask + x * (1 - road_mask))[0]
    return InferenceLoop.to_uint8_hwc(out) if as_uint8 else out


def count_launches(fn):
    """Device kernels and memcpys one call of fn enqueues, or None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev_type = getattr(torch.autograd.DeviceType, "CUDA")
        n = sum(1 for e in prof.events() if e.device_type == dev_type)
        return n or None
    except Exception as e:  # noqa: BLE001 -- a count is informational; the timing stands without it
        print("launch count not available: %r" % (e,), file=sys.stderr)
        return None


def ab(sides, calls, blocks):
    """{name: median ms per call}, and the per-block values; the sides alternate block by block."""
    for fn in sides.values():
        for _ in range(2):
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
    wall = {name: [] for name in sides}
    for _ in range(blocks):
        for name, fn in sides.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            wall[name].append(1e3 * (time.perf_counter() - t0) / calls)
    return {name: round(statistics.median(v), 5) for name, v in wall.items()}, {name: [round(x, 5) for x in v] for name, v in wall.items()}


def compare(img, ins_dev, w33):
    """The device result against the torch-ops result on the same inputs."""
    t_f, d_f = torch_finish(img, ins_dev, w33, False), finish.road_blur(img, ins_dev, ROAD)
    t_u, d_u = torch_finish(img, ins_dev, w33, True), finish.road_blur(img, ins_dev, ROAD, as_uint8=True)
    road = (ins_dev == ROAD)[None].expand_as(img)
    same_off_road = bool(torch.equal(d_f[~road].view(torch.int32), img[~road].view(torch.int32)))
    # two float32 evaluations of nine terms: each within gamma_9 * sum|w x| of the exact sum
    sa = F.conv2d(F.pad(img[None].abs().double(), (1, 1, 1, 1), mode="reflect"), w33.double(), groups=3)[0]
    g9 = 9 * 2.0 ** -24 / (1 - 9 * 2.0 ** -24)
    within = bool(((d_f.double() - t_f.double()).abs()[road] <= 2 * g9 * sa[road]).all())
    byte_diff = int((t_u.int() - d_u.int()).abs().max())
    return {"non_road_bit_for_bit": same_off_road, "road_within_two_gamma9": within, "max_byte_difference": byte_diff}


def kernel_part(dev, args):
    w33 = finish.gaussian_kernel2d(3, 2.0).to(dev)[None, None].expand(3, 1, 3, 3).contiguous()
    out = []
    for (W, H) in ((960, 540), (1408, 376)):
        gen = torch.Generator().manual_seed(W)
        img = (torch.rand((3, H, W), generator=gen) * 2.4 - 1.2).to(dev)
        for frac in (0.0, 0.3, 1.0):
            ins_np = np.where(np.random.default_rng(H).random((H, W)) < frac, ROAD, 3).astype(np.int16)
            ins_dev = torch.from_numpy(ins_np).to(dev)
            rec = {"image": [W, H], "road_fraction": frac, "check": compare(img, ins_dev, w33)}
            for as_u8, key in ((False, "float"), (True, "uint8")):
                sides = {"torch": lambda: torch_finish(img, ins_dev, w33, as_u8),
                         "torch_numpy_map": lambda: torch_finish(img, ins_np, w33, as_u8),
                         "device": lambda: finish.road_blur(img, ins_dev, ROAD, as_uint8=as_u8)}
                med, blocks = ab(sides, args.calls, args.blocks)
                rec[key] = {"ms_per_call": med, "torch_over_device": round(med["torch"] / med["device"], 2),
                            "torch_numpy_map_over_device": round(med["torch_numpy_map"] / med["device"], 2),
                            "ms_blocks": blocks}
            out.append(rec)
            print(json.dumps({k: (v if k in ("image", "road_fraction", "check") else {"ms_per_call": v["ms_per_call"]}) for k, v in rec.items()}), flush=True)
    # launches, in a pass of their own (960 x 540, 30 % road)
    W, H = 960, 540
    img = (torch.rand((3, H, W)) * 2.4 - 1.2).to(dev)
    ins_np = np.where(np.random.default_rng(1).random((H, W)) < 0.3, ROAD, 3).astype(np.int16)
    ins_dev = torch.from_numpy(ins_np).to(dev)
    launches = {}
    for as_u8, key in ((False, "float"), (True, "uint8")):
        launches[key] = {"torch": count_launches(lambda: torch_finish(img, ins_dev, w33, as_u8)),
                         "torch_numpy_map": count_launches(lambda: torch_finish(img, ins_np, w33, as_u8)),
                         "device": count_launches(lambda: finish.road_blur(img, ins_dev, ROAD, as_uint8=as_u8))}
    return out, launches


def loop_part(dev, args):
    from gaussiancity_amd.rasterizer import GaussianRasterizerWrapper
    n_pts = 518400
    cfg, sc = synth.make_scene("C4", n_pts)
    W, H = cfg["W"], cfg["H"]
    wr = GaussianRasterizerWrapper(synth.intrinsics(W, H), (W, H), device=dev)
    rot = np.zeros((n_pts, 4), np.float32)
    rot[:, 0] = 1.0
    pts_np = np.concatenate([sc["means3D"], np.ones((n_pts, 1), np.float32), sc["scales"], rot, sc["colors_precomp"]], axis=1)
    points = torch.from_numpy(pts_np.astype(np.float32)).to(dev)
    orbit = synth.orbit_poses()
    ins_dev = torch.from_numpy(np.where(np.random.default_rng(2).random((H, W)) < 0.3, ROAD, 3).astype(np.int16)).to(dev)
    render = lambda p, cp, cq: wr(p, cp, cq)  # noqa: E731
    loops = {
        "to_uint8_hwc": InferenceLoop(render, device=dev),
        "finish_fn": InferenceLoop(render, device=dev, finish_fn=lambda i, im: finish.road_blur(im, ins_dev, ROAD, as_uint8=True)),
        "blend_kernel_bytes": InferenceLoop(render, device=dev, render_uint8_fn=lambda p, cp, cq: wr(p, cp, cq, as_uint8=True)),
    }
    sink = [0]

    def consume(i, frame):
        sink[0] += int(frame[0, 0, 0])

    def run(loop, n):
        with torch.no_grad():
            loop.run(points, [orbit[i % len(orbit)] for i in range(n)], consume=consume)

    for loop in loops.values():
        run(loop, 48)
    wall = {name: [] for name in loops}
    for _ in range(args.blocks):
        for name, loop in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(loop, args.frames)
            torch.cuda.synchronize()
            wall[name].append(1e3 * (time.perf_counter() - t0) / args.frames)
    med = {name: round(statistics.median(v), 5) for name, v in wall.items()}
    return {"workload": "%d points [N,14], %dx%d, 24-pose orbit, uint8 frames to pinned host memory, 3 streams" % (n_pts, W, H),
            "road_fraction": 0.3, "frames_per_block": args.frames, "ms_per_frame": med,
            "finish_fn_minus_to_uint8_hwc_ms": round(med["finish_fn"] - med["to_uint8_hwc"], 5),
            "finish_fn_over_to_uint8_hwc": round(med["finish_fn"] / med["to_uint8_hwc"], 3),
            "ms_blocks": {name: [round(x, 5) for x in v] for name, v in wall.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="calls per timed block of the kernel part")
    ap.add_argument("--frames", type=int, default=96, help="frames per timed block of the loop part")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_finish.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finish_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    cases, launches = kernel_part(dev, args)
    rec = {"tool": "tools/finish_bench.py", "device": torch.cuda.get_device_name(0),
           "timing": "host wall time per call around blocks of %d calls ending in a synchronise; all sides in one process on "
                     "one stream, alternating; median of %d blocks" % (args.calls, args.blocks),
           "kernel_size": 3, "sigma": 2.0, "cases": cases, "launches_per_frame_960x540": launches,
           "native_calls": finish.stats()["native_calls"]}
    if not args.skip_loop:
        rec["inference_loop"] = loop_part(dev, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "cases"}))
    if not all(c["check"]["non_road_bit_for_bit"] and c["check"]["road_within_two_gamma9"] and c["check"]["max_byte_difference"] <= 1
               for c in cases):
        raise SystemExit("device and torch results differ")


if __name__ == "__main__":
    main()
