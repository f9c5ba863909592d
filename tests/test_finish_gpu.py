"""-m gpu: the frame-finish kernel (gaussiancity_amd.finish -> gcv_frame_finish, include/gcv.h K19) against the float64
restatement of tests/finish_ref.py, with the same float32 weights cast to float64.

Road pixels: |out - ref64| <= gamma_n * sum |w x|, n = (2r+1)^2 (one product rounding and at most n - 1 addition roundings
per term: derived, not measured).  Every other pixel: the input bit for bit.  Bytes: within 1 of the float64 frame's byte,
and a difference of 1 only next to an integer boundary (finish_ref.check_bytes)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import finish_ref as R
from gaussiancity_amd import finish
from gaussiancity_amd.frames import InferenceLoop

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _weights(k, sigma=2.0):
    return finish.gaussian_kernel2d(k, sigma).numpy()


@functools.lru_cache(maxsize=None)
def _case(h, w, k, mask):
    """(img float32 [3,H,W], map int16 [H,W], out64, road, bound): computed once, shared, never changed."""
    img, m = R.image(h, w), R.make_mask(mask, h, w)
    m.setflags(write=False)
    return (img, m) + R.finish64(img, m, _weights(k))


def _dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)   # (a copy: the shared arrays are read-only)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("h,w,k", R.SHAPES, ids=lambda v: str(v))
def test_float_and_bytes_against_float64(cuda_device, h, w, k):
    before = finish.stats()
    for mask in R.MASKS:
        img, m, out64, road, bound = _case(h, w, k, mask)
        what = "%dx%d k%d %s" % (h, w, k, mask)
        dimg, dmap = _dev(img, cuda_device), _dev(m, cuda_device)
        keep = dimg.clone()
        got = finish.road_blur(dimg, dmap, R.ROAD, kernel_size=k)
        assert got.shape == dimg.shape and got.dtype == torch.float32 and got.is_cuda and got.is_contiguous()
        R.check_float(got.cpu().numpy(), img, out64, road, bound, what)
        if mask == "none":
            assert torch.equal(_bits(got), _bits(dimg)), what + ": no road, yet the frame changed"
        assert torch.equal(_bits(dimg), _bits(keep)), what + ": the input was written"
        # bytes: the same call's float output through to_uint8_hwc, byte for byte; BGR the channel axis reversed
        u8 = finish.road_blur(dimg, dmap, R.ROAD, kernel_size=k, as_uint8=True)
        assert tuple(u8.shape) == (h, w, 3) and u8.dtype == torch.uint8 and u8.is_contiguous()
        want = InferenceLoop.to_uint8_hwc(got)
        assert torch.equal(u8, want), what + ": bytes differ from to_uint8_hwc of the float output"
        bgr = finish.road_blur(dimg, dmap, R.ROAD, kernel_size=k, as_uint8=True, bgr=True)
        assert torch.equal(bgr, want.flip(-1)), what + ": BGR bytes"
        R.check_bytes(u8.cpu().numpy(), out64, bound, what=what)
        R.check_bytes(bgr.cpu().numpy(), out64, bound, bgr=True, what=what + " bgr")
    after = finish.stats()
    assert after["native_calls"] == before["native_calls"] + 3 * len(R.MASKS) and after["fallback_calls"] == before["fallback_calls"]


def test_float64_reference_with_itself_uses_no_allowance():
    img, m, out64, road, bound = _case(37, 70, 3, "random30")
    own = np.floor(R.byte64(out64)).astype(np.uint8).transpose(0, 2, 3, 1)
    assert R.check_bytes(own, out64, bound, what="float64 with itself") == 0


def test_flip_and_road_id(cuda_device):
    img, m, *_ = _case(37, 70, 3, "random30")
    dimg, dmap = _dev(img, cuda_device), _dev(m, cuda_device)
    a = finish.road_blur(dimg, dmap, R.ROAD, flip_mask_lr=True)
    b = finish.road_blur(dimg, dmap.flip(-1), R.ROAD)
    assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(_bits(a), _bits(finish.road_blur(dimg, dmap, R.ROAD)))
    out64, road, bound = R.finish64(img, m, _weights(3), flip=True)
    R.check_float(a.cpu().numpy(), img, out64, road, bound, "flipped mask")
    for absent in (11, -3, 32767):
        assert torch.equal(_bits(finish.road_blur(dimg, dmap, absent)), _bits(dimg))
    # another id: 257 shares its low byte with ROAD and is in the map
    out64, road, bound = R.finish64(img, m, _weights(3), road_id=257)
    assert road.any()
    R.check_float(finish.road_blur(dimg, dmap, 257).cpu().numpy(), img, out64, road, bound, "road id 257")
    # a map of another integer dtype, and one on the host as upstream has it
    want = finish.road_blur(dimg, dmap, R.ROAD)
    assert torch.equal(_bits(finish.road_blur(dimg, dmap.long(), R.ROAD)), _bits(want))
    assert torch.equal(_bits(finish.road_blur(dimg, m.copy(), R.ROAD)), _bits(want))


@pytest.mark.parametrize("k", [3, 5])
def test_batch(cuda_device, k):
    h, w, b = 37, 70, 3
    img = R.image(h, w, b=b)
    maps = np.stack([R.make_mask("random30", h, w, seed=s) for s in range(b)])
    dimg, dmaps = _dev(img, cuda_device), _dev(maps, cuda_device)
    for dm, ref_maps in ((dmaps[1], maps[1]), (dmaps, maps)):                # one shared map; a map per image
        got = finish.road_blur(dimg, dm, R.ROAD, kernel_size=k)
        u8 = finish.road_blur(dimg, dm, R.ROAD, kernel_size=k, as_uint8=True, bgr=True)
        assert tuple(got.shape) == (b, 3, h, w) and tuple(u8.shape) == (b, h, w, 3)
        for i in range(b):
            mi = dm if dm.dim() == 2 else dm[i]
            assert torch.equal(_bits(got[i]), _bits(finish.road_blur(dimg[i], mi, R.ROAD, kernel_size=k)))
            assert torch.equal(u8[i], finish.road_blur(dimg[i], mi, R.ROAD, kernel_size=k, as_uint8=True, bgr=True))
        out64, road, bound = R.finish64(img, ref_maps, _weights(k))
        R.check_float(got.cpu().numpy(), img, out64, road, bound, "batch k%d maps %s" % (k, tuple(dm.shape)))


def test_strides(cuda_device):
    h, w, b = 37, 70, 2
    gen = torch.Generator().manual_seed(9)
    wide = (torch.rand((b, 4, h + 5, 2 * w + 3), generator=gen) * 3 - 1.5).to(cuda_device)
    dmap = torch.from_numpy(R.make_mask("random30", h, w)).to(cuda_device)
    view = wide[:, 1:4, 2:2 + h, 3:3 + w]                                   # row stride 2W + 3, channel stride (H + 5)(2W + 3)
    assert view.stride(3) == 1 and view.stride(2) != w and view.stride(1) != h * w and not view.is_contiguous()
    keep = wide.clone()
    want = finish.road_blur(view.contiguous(), dmap, R.ROAD)
    assert torch.equal(_bits(finish.road_blur(view, dmap, R.ROAD)), _bits(want))
    assert torch.equal(finish.road_blur(view, dmap, R.ROAD, as_uint8=True), finish.road_blur(view.contiguous(), dmap, R.ROAD, as_uint8=True))
    assert torch.equal(_bits(finish.road_blur(view[0], dmap, R.ROAD)), _bits(want[0]))
    # pixel stride 2 (a contiguous copy inside), channels last, and an expanded batch (batch stride 0)
    for odd in (wide[:, 1:4, 2:2 + h, 0:2 * w:2], view.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), view[0].expand(3, 3, h, w)):
        assert torch.equal(_bits(finish.road_blur(odd, dmap, R.ROAD)), _bits(finish.road_blur(odd.contiguous(), dmap, R.ROAD)))
    assert torch.equal(_bits(wide), _bits(keep))
    out64, road, bound = R.finish64(view.cpu().numpy(), dmap.cpu().numpy(), _weights(3))
    R.check_float(want.cpu().numpy(), view.cpu().numpy(), out64, road, bound, "strided view")


def test_determinism_and_tiling(cuda_device):
    for k in (3, 7):
        r = k // 2
        img, m = R.image(65, 129), R.make_mask("random30", 65, 129)
        dimg, dmap = _dev(img, cuda_device), _dev(m, cuda_device)
        full = finish.road_blur(dimg, dmap, R.ROAD, kernel_size=k)
        assert torch.equal(_bits(full), _bits(finish.road_blur(dimg, dmap, R.ROAD, kernel_size=k)))
        crop = finish.road_blur(dimg[:, :37, :70], dmap[:37, :70], R.ROAD, kernel_size=k)   # other block and lane positions
        assert torch.equal(_bits(full[:, :37 - r, :70 - r]), _bits(crop[:, :37 - r, :70 - r]))
        shifted = finish.road_blur(dimg[:, 5:, 9:], dmap[5:, 9:], R.ROAD, kernel_size=k)     # every pixel in another lane and block
        assert torch.equal(_bits(full[:, 5 + r:, 9 + r:]), _bits(shifted[:, r:, r:]))


def test_both_outputs_in_one_launch_through_the_c_abi(cuda_device):
    from gaussiancity_amd import _native_v as V
    from gaussiancity_amd._loader import current_stream
    h, w, b, k = 65, 129, 2, 5
    img = R.image(h, w, b=b)
    maps = np.stack([R.make_mask("checker", h, w), R.make_mask("random30", h, w)])
    dimg, dmaps = _dev(img, cuda_device), _dev(maps, cuda_device)
    wts = np.ascontiguousarray(_weights(k)).reshape(-1)
    warr = (C.c_float * wts.size)(*wts.tolist())
    for bgr in (0, 1):
        # one allocation, the outputs directly behind the image: neighbours are not an overlap
        buf = torch.empty(2 * dimg.numel(), dtype=torch.float32, device=cuda_device)
        src, out_f = buf[:dimg.numel()].view_as(dimg), buf[dimg.numel():].view_as(dimg)
        src.copy_(dimg)
        out_f.fill_(float("nan"))
        out_u = torch.full((b, h, w, 3), 77, dtype=torch.uint8, device=cuda_device)
        V.check(V.lib().gcv_frame_finish(src.data_ptr(), 3 * h * w, h * w, w, b, h, w, dmaps.data_ptr(), h * w, R.ROAD, 0, k // 2,
                                         warr, out_f.data_ptr(), out_u.data_ptr(), bgr, current_stream()), "gcv_frame_finish")
        assert torch.equal(_bits(out_f), _bits(finish.road_blur(dimg, dmaps, R.ROAD, kernel_size=k)))
        assert torch.equal(out_u, finish.road_blur(dimg, dmaps, R.ROAD, kernel_size=k, as_uint8=True, bgr=bool(bgr)))
        assert torch.equal(_bits(src), _bits(dimg))
        f2, u2 = finish.frame_finish(dimg, dmaps, R.ROAD, kernel_size=k, bgr=bool(bgr))
        assert torch.equal(_bits(f2), _bits(out_f)) and torch.equal(u2, out_u)
    # in place is refused before anything is queued
    assert V.lib().gcv_frame_finish(src.data_ptr(), 3 * h * w, h * w, w, b, h, w, dmaps.data_ptr(), h * w, R.ROAD, 0, k // 2, warr,
                                    src.data_ptr(), None, 0, current_stream()) == -1
    assert b"overlap" in V.lib().gcv_last_error()


def test_refusals_on_the_device(cuda_device):
    img = torch.zeros(3, 8, 8, device=cuda_device)
    m = torch.zeros(8, 8, dtype=torch.int16, device=cuda_device)
    with pytest.raises(TypeError):
        finish.road_blur(img.half(), m, 1)
    with pytest.raises(ValueError):
        finish.road_blur(img[:, :3], m[:3], 1, kernel_size=7)
    with pytest.raises(RuntimeError):
        finish.road_blur(img.clone().requires_grad_(True), m, 1)


def test_end_to_end_small(cuda_device):
    """A layout scene through visible_point_map (a real int16 ins_map with roads) and the rasterizer wrapper at a 96 x 64
    sensor: the finished bytes hold the rules above against the float64 restatement on the wrapper's float image, agree
    with the torch formulation on it, and differ from the wrapper's own as_uint8 bytes on road pixels only."""
    from gaussiancity_amd import points as P
    from gaussiancity_amd import synth
    from gaussiancity_amd.rasterizer import GaussianRasterizerWrapper
    size, W, H = 96, 96, 64
    L = synth.s_layout(size, 77, block=24, road=6, max_height=20)
    inv = {v: k for k, v in synth.LAYOUT_CLASSES.items()}
    maps = [torch.from_numpy(L[k]).to(cuda_device) for k in ("INS", "TD_HF", "BU_HF", "PTS")]
    rows = P.extrude_points(True, inv, synth.LAYOUT_SCALES, synth.LAYOUT_SEG_INS, *maps)
    rig, cam_pos, cam_quat = synth.layout_camera(size, W=W, H=H, pose=0)   # a third of this view is road
    ins_map = P.visible_point_map(rows, rig, cam_pos.copy(), cam_quat, 0)[1]
    assert ins_map.dtype == torch.int16 and tuple(ins_map.shape) == (H, W) and ins_map.is_cuda
    road_id = synth.LAYOUT_CLASSES["ROAD"]
    road = (ins_map == road_id)
    n_road = int(road.sum())
    assert 0 < n_road < H * W, "the pose must show a road and something else, got %d road pixels" % n_road
    n = int(rows.shape[0])
    gen = torch.Generator().manual_seed(5)
    pts = torch.zeros((n, 14), dtype=torch.float32)
    pts[:, 0:3] = rows[:, 0:3].float().cpu()
    pts[:, 3] = 1.0
    pts[:, 4:7] = rows[:, 3:4].float().cpu() * 0.45
    pts[:, 7] = 1.0
    pts[:, 11:14] = torch.rand((n, 3), generator=gen) * 2 - 1
    pts = pts.to(cuda_device)
    wr = GaussianRasterizerWrapper(synth.intrinsics(W, H), (W, H), device=cuda_device)
    with torch.no_grad():
        img = wr(pts, cam_pos, cam_quat)
        plain = wr(pts, cam_pos, cam_quat, as_uint8=True)
        got = finish.road_blur(img, ins_map, road_id, as_uint8=True)
    assert tuple(img.shape) == (3, H, W) and tuple(got.shape) == (H, W, 3)
    out64, road64, bound = R.finish64(img.cpu().numpy(), ins_map.cpu().numpy(), _weights(3), road_id=road_id)
    R.check_bytes(got.cpu().numpy(), out64, bound, what="end to end")
    # the torch formulation on the same float image (the CPU path of road_blur): within one byte, and equal off the road
    torch_u8 = finish.road_blur(img.cpu(), ins_map.cpu(), road_id, as_uint8=True)
    R.check_bytes(torch_u8.numpy(), out64, bound, what="end to end, torch formulation")
    assert int((got.cpu().int() - torch_u8.int()).abs().max()) <= 1
    assert torch.equal(got.cpu()[~road.cpu()], torch_u8[~road.cpu()])
    changed = (got != plain).any(dim=-1)
    assert bool((changed & road).any()), "the blur changed no road pixel"
    assert not bool((changed & ~road).any()), "a non-road pixel changed"
    # finished inside the frame loop
    loop = InferenceLoop(lambda p, cp, cq: wr(p, cp, cq), device=cuda_device,
                         finish_fn=lambda i, im: finish.road_blur(im, ins_map, road_id, as_uint8=True))
    with torch.no_grad():
        frames = loop.run(pts, [(cam_pos, cam_quat)] * 4)
    assert len(frames) == 4 and all(np.array_equal(f, got.cpu().numpy()) for f in frames)
