"""Frame finish without a GPU (include/gcv.h K19, gaussiancity_amd/finish.py): the library's two entry points and every
argument error, the weight table against an independent float64 evaluation, the CPU path of road_blur against the
float64 restatement of tests/finish_ref.py, and InferenceLoop's finish_fn."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import finish_ref as R
from gaussiancity_amd import _native_v as V
from gaussiancity_amd import finish
from gaussiancity_amd.frames import InferenceLoop

INVALID = -1  # GCV_ERR_INVALID_ARGUMENT


def test_library_exports_the_entry_points():
    lib = V.lib()
    assert {"gcv_frame_finish", "gcv_frame_finish_radius_max"} <= set(V.EXPORTED_SYMBOLS)
    assert lib.gcv_frame_finish_radius_max() == 3


def _call(lib, **over):
    """gcv_frame_finish with plausible (never dereferenced) arguments for a contiguous 1 x 3 x 8 x 8 image, some replaced."""
    w = (C.c_float * 49)(*([1.0 / 9] * 49))
    a = dict(img=0x100000, bs=192, cs=64, rs=8, batch=1, h=8, w=8, map=0x200000, mbs=0, road=1, flip=0, radius=1,
             weights=w, out_f32=0x300000, out_u8=0x400000, bgr=0)
    a.update(over)
    return lib.gcv_frame_finish(a["img"], a["bs"], a["cs"], a["rs"], a["batch"], a["h"], a["w"], a["map"], a["mbs"], a["road"],
                                a["flip"], a["radius"], a["weights"], a["out_f32"], a["out_u8"], a["bgr"], None)


@pytest.mark.parametrize("over,word", [
    (dict(img=None), b"null"), (dict(map=None), b"null"), (dict(weights=None), b"null"),
    (dict(out_f32=None, out_u8=None), b"null"),
    (dict(radius=0), b"radius"), (dict(radius=4), b"radius"), (dict(radius=-1), b"radius"),
    (dict(h=1), b"reflect"), (dict(w=1), b"reflect"), (dict(h=3, radius=3), b"reflect"), (dict(w=2, radius=2), b"reflect"),
    (dict(h=0), b"positive"), (dict(w=-4), b"positive"), (dict(batch=0), b"positive"),
    (dict(out_f32=0x100000), b"overlap"), (dict(out_f32=0x100000 + 4 * 191), b"overlap"),
    (dict(out_f32=0x100000 - 4 * 191), b"overlap"), (dict(bs=4096, batch=2, out_f32=0x100000 + 4 * 4096), b"overlap"),
], ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_argument_errors_come_back_before_anything_is_queued(over, word):
    """No GPU is present here: a call that got as far as a launch would report a HIP error (-2), not -1."""
    lib = V.lib()
    assert _call(lib, **over) == INVALID
    msg = lib.gcv_last_error()
    assert b"gcv_frame_finish" in msg and word in msg, msg


def _kernel64(k, sigma):
    sx, sy = (sigma, sigma) if isinstance(sigma, float) else sigma

    def k1(s):
        pdf = [math.exp(-0.5 * ((i - (k - 1) / 2.0) / s) ** 2) for i in range(k)]
        return [p / math.fsum(pdf) for p in pdf]
    ky, kx = k1(sy), k1(sx)
    return np.array([[a * b for b in kx] for a in ky], np.float64)


@pytest.mark.parametrize("k,sigma", [(3, 2.0), (5, 1.0), (7, (0.5, 3.0))])
def test_gaussian_kernel2d_against_float64(k, sigma):
    """The float32 recipe against the same recipe in float64.  Where a correctly rounded float32 result can sit: per axis
    x / sigma is one rounding, its square a second, so the exponent a = 0.5 (x / sigma)^2 carries a relative error of
    3u and exp(-a) one of 3 a u plus exp's own (2u allowed); the k-term sum adds (k - 1) u, the division u; the outer
    product adds the two axes' errors and one more rounding.  With a <= a_max = 0.5 ((k - 1) / 2 / min sigma)^2 that is
    (2 (3 a_max + k + 2) + 1) u relative, plus the final rounding of the float64 value to float32 (u)."""
    got = finish.gaussian_kernel2d(k, sigma)
    assert got.dtype == torch.float32 and tuple(got.shape) == (k, k)
    want = _kernel64(k, sigma)
    smin = sigma if isinstance(sigma, float) else min(sigma)
    a_max = 0.5 * ((k - 1) / 2.0 / smin) ** 2
    rel = (2 * (3 * a_max + k + 2) + 2) * R.U
    err = np.abs(got.double().numpy() - want) / want
    print("k=%d sigma=%r: max relative error %.3g u, bound %.3g u" % (k, sigma, err.max() / R.U, rel / R.U))
    assert np.all(err <= rel)
    g = got.numpy()
    assert np.array_equal(g, g[::-1, ::-1]) and np.array_equal(g, g[::-1]) and np.array_equal(g, g[:, ::-1])
    if not isinstance(sigma, tuple):
        assert np.array_equal(g, g.T)
    assert abs(float(got.double().sum()) - 1.0) <= 4 * R.U
    if (k, sigma) == (3, 2.0):
        assert round(float(got[1, 1]), 4) == 0.1308 and round(float(got[0, 0]), 4) == 0.1019
    again = finish.gaussian_kernel2d(k, sigma)
    again[0, 0] = 5.0                               # a copy: the cached table is not the caller's to edit
    assert torch.equal(finish.gaussian_kernel2d(k, sigma), got)


@pytest.mark.parametrize("h,w,k", R.SHAPES, ids=lambda v: str(v))
def test_cpu_path_against_float64(h, w, k):
    img = R.image(h, w)
    wts = finish.gaussian_kernel2d(k, 2.0).numpy()
    before = finish.stats()["fallback_calls"]
    for name in R.MASKS:
        m = R.make_mask(name, h, w)
        out64, road, bound = R.finish64(img, m, wts)
        got = finish.road_blur(torch.from_numpy(img.copy()), torch.from_numpy(m), R.ROAD, kernel_size=k)
        R.check_float(got.numpy(), img, out64, road, bound, "cpu %dx%d k%d %s" % (h, w, k, name))
        if name == "none":
            assert np.array_equal(got.numpy().view(np.int32), img.view(np.int32))
        for bgr in (False, True):
            u8 = finish.road_blur(torch.from_numpy(img.copy()), torch.from_numpy(m), R.ROAD, kernel_size=k, as_uint8=True, bgr=bgr)
            assert u8.dtype == torch.uint8 and tuple(u8.shape) == (h, w, 3)
            want = InferenceLoop.to_uint8_hwc(got)
            assert torch.equal(u8, want.flip(-1) if bgr else want)
    assert finish.stats()["fallback_calls"] == before + 3 * len(R.MASKS) and finish.stats()["native_calls"] == 0
    assert R.check_bytes(np.floor(R.byte64(out64)).astype(np.uint8).transpose(0, 2, 3, 1), out64, bound, what="float64 with itself") == 0


def test_cpu_path_shapes_flip_batch_and_maps():
    h, w = 6, 9
    img = torch.from_numpy(R.image(h, w, b=3).copy())
    maps = torch.from_numpy(np.stack([R.make_mask("random30", h, w, seed=s) for s in range(3)]))
    wts = finish.gaussian_kernel2d(3, 2.0).numpy()
    got = finish.road_blur(img, maps, R.ROAD)
    out64, road, bound = R.finish64(img.numpy(), maps.numpy(), wts)
    R.check_float(got.numpy(), img.numpy(), out64, road, bound, "cpu batch with [B,H,W] maps")
    for b in range(3):
        assert torch.equal(finish.road_blur(img[b], maps[b], R.ROAD), got[b])
    shared = finish.road_blur(img, maps[0], R.ROAD)
    assert all(torch.equal(finish.road_blur(img[b], maps[0], R.ROAD), shared[b]) for b in range(3))
    assert torch.equal(finish.road_blur(img, maps, R.ROAD, flip_mask_lr=True), finish.road_blur(img, maps.flip(-1), R.ROAD))
    assert torch.equal(finish.road_blur(img, maps, 12345), img)
    for dt in (torch.int32, torch.int64, torch.uint8):   # any integer dtype; numpy as upstream has it
        assert torch.equal(finish.road_blur(img, maps.clamp(0, 100).to(dt), R.ROAD), finish.road_blur(img, maps.clamp(0, 100), R.ROAD))
    assert torch.equal(finish.road_blur(img, maps.numpy(), R.ROAD), got)
    f, u = finish.frame_finish(img, maps, R.ROAD)
    assert torch.equal(f, got) and torch.equal(u, finish.road_blur(img, maps, R.ROAD, as_uint8=True))
    keep = img.clone()
    finish.road_blur(img, maps, R.ROAD)
    assert torch.equal(img, keep)


def test_refusals():
    img, m = torch.zeros(3, 4, 4), torch.zeros(4, 4, dtype=torch.int16)
    with pytest.raises(TypeError):
        finish.road_blur(img.double(), m, 1)
    with pytest.raises(TypeError):
        finish.road_blur(img.half(), m, 1)
    with pytest.raises(TypeError):
        finish.road_blur(img, m.float(), 1)
    with pytest.raises(ValueError):
        finish.road_blur(torch.zeros(3, 1, 4), torch.zeros(1, 4, dtype=torch.int16), 1)      # H <= radius
    with pytest.raises(ValueError):
        finish.road_blur(torch.zeros(3, 3, 8), torch.zeros(3, 8, dtype=torch.int16), 1, kernel_size=7)  # H == radius
    with pytest.raises(ValueError):
        finish.road_blur(img, m, 1, kernel_size=4)
    with pytest.raises(ValueError):
        finish.road_blur(img, m, 1, kernel_size=9)
    with pytest.raises(ValueError):
        finish.road_blur(img, torch.zeros(5, 4, dtype=torch.int16), 1)
    with pytest.raises(ValueError):
        finish.road_blur(torch.zeros(4, 4), m, 1)
    with pytest.raises(ValueError):
        finish.road_blur(img, m, 1, sigma=0.0)
    leaf = torch.zeros(3, 4, 4, requires_grad=True)
    with pytest.raises(RuntimeError):
        finish.road_blur(leaf, m, 1)
    with torch.no_grad():
        assert not finish.road_blur(leaf, m, 1).requires_grad


def test_inference_loop_finish_fn():
    gen = torch.Generator().manual_seed(3)
    frames = [torch.rand(3, 5, 7, generator=gen) * 3 - 1.5 for _ in range(5)]
    maps = [torch.from_numpy(R.make_mask("random30", 5, 7, seed=i)) for i in range(5)]
    poses = [(i, None) for i in range(5)]

    def render(points, cam_pos, cam_quat):
        return frames[cam_pos]

    plain = InferenceLoop(render, n_streams=2).run(None, poses)
    assert all(np.array_equal(f, InferenceLoop.to_uint8_hwc(frames[i]).numpy()) for i, f in enumerate(plain))
    none = InferenceLoop(render, n_streams=2, finish_fn=None).run(None, poses)
    assert all(np.array_equal(a, b) for a, b in zip(plain, none))
    seen = []

    def fin(i, img):
        seen.append(i)
        return finish.road_blur(img, maps[i], R.ROAD, as_uint8=True)

    done = InferenceLoop(render, n_streams=2, finish_fn=fin).run(None, poses)
    assert seen == list(range(5)) and len(done) == 5
    for i, f in enumerate(done):
        assert np.array_equal(f, finish.road_blur(frames[i], maps[i], R.ROAD, as_uint8=True).numpy())
    assert any(not np.array_equal(a, b) for a, b in zip(plain, done))
    with pytest.raises(ValueError):
        InferenceLoop(render, finish_fn=fin, render_uint8_fn=lambda p, a, b: None)
