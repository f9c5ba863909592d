"""-m gpu: the frame mode "tile ids" (option "blend_ranks", gcr_api.hip enqueue_render_lds): the scatter writes 4-byte
Gaussian indices, the per-tile sort kernel is not launched and the forward blend ranks its own tile by the depth in the
records it gathers.  The order is the one of the (depth << 32 | index) keys, so with the option on and off a frame is
the same bit for bit -- image, radii, final_T, n_contrib, num_rendered, the sorted per-tile lists -- and the oracle's.

Scenes (a few thousand Gaussians, 128 x 96 at the most):
  * "stack": small Gaussians stacked on the centres of a 128 x 96 image's tiles so that the tile lists have 0, 1, 2, 63,
    64, 65 (the 64-key chunks of the rank), 128, 129, 223, 224 (one blend chunk / the first list that is ranked from the
    depths alone), 600, 1024 (the last list ranked in LDS) and 1100 entries (ranked through global memory: only
    reachable with a stale length hint, which the test hands in), many of them at equal depth;
  * "ties": every Gaussian at one of three depths in the same tiles -- ties resolve by ascending index;
  * "edge": 70 x 45 pixels, partial tiles on both edges, lists beyond a chunk.
Every frame goes through the staged C ABI with buffers of the test's own, and the mode the host chose is read back
(option "last_tile_ids") -- otherwise both runs might take the same path."""
import ctypes as C

import numpy as np
import pytest
import torch

import gpu_util as G
import scenes
from test_gpu_async import _args
from test_gpu_parity import _check_grads, _frame

pytestmark = pytest.mark.gpu

STACK_LENGTHS = (0, 1, 2, 63, 64, 65, 128, 129, 223, 224, 600, 1024, 1100)


def _stack_scene(rs, W, H, lengths, seed):
    """len(lengths) tiles of the image, tile k with lengths[k] small Gaussians on its centre pixel (a radius of three
    pixels: inside the tile), at view depths 60 + 0.25 * (j % 9): nine depth classes per tile, ties inside each."""
    rng = np.random.default_rng(seed)
    gx = (W + 15) // 16
    view = rs.view_matrix.cpu().numpy().astype(np.float64)  # row vectors: p_view = [p, 1] @ view
    inv = np.linalg.inv(view)
    pts, tiles = [], []
    step = 3  # every third tile: the stacks do not touch each other's tiles
    for k, n in enumerate(lengths):
        t = (k * step) % (gx * ((H + 15) // 16))
        tx, ty = t % gx, t // gx
        px, py = tx * 16 + 8.0, ty * 16 + 8.0
        ndc_x, ndc_y = (2 * px + 1) / W - 1, (2 * py + 1) / H - 1
        for j in range(n):
            z = 60.0 + 0.25 * (j % 9)
            pv = np.array([-ndc_x * rs.tanfovx * z, -ndc_y * rs.tanfovy * z, z, 1.0])  # (the wrapper's view looks down -x, -y)
            pts.append((pv @ inv)[:3])
        tiles.append((t, n))
    P = len(pts)
    order = rng.permutation(P)  # index order unrelated to tile and depth
    xyz = np.asarray(pts, np.float32)[order]
    M = 4
    shs = np.zeros((P, M, 3), np.float32)
    shs[:, 0] = rng.normal(0.3, 0.8, (P, 3))
    rot = np.zeros((P, 4), np.float32)
    rot[:, 0] = 1.0
    sc = dict(means3D=xyz, scales=np.full((P, 3), 0.02, np.float32), rotations=rot,
              opacities=rng.uniform(0.003, 0.03, (P, 1)).astype(np.float32),
              colors_precomp=rng.uniform(-1, 1, (P, 3)).astype(np.float32), shs=shs, sh_degree=1)
    return sc, tiles


_made = {}


def _make(name, O):
    """(P, W, H, settings, scene, the oracle's frame, length hint or None): computed once, shared, never changed."""
    if name in _made:
        return _made[name]
    hint = None
    if name == "stack":
        W, H = 128, 96
        rs = scenes.camera(W, H)._replace(sh_degree=1, bg=torch.tensor((0.1, 0.2, 0.3)))
        sc, tiles = _stack_scene(rs, W, H, STACK_LENGTHS, 5)
        fr = _frame(O, rs, sc)
        n = fr.ranges[:, 1].astype(np.int64) - fr.ranges[:, 0]
        for t, want in tiles:
            assert n[t] == want, (t, int(n[t]), want)
        assert int(fr.n_contrib.max()) > 224  # pixels that walk into the second chunk of a long list
        hint = 300  # stale: the frame takes the mode of short lists although three of its lists are longer
    elif name == "ties":
        W, H = 80, 64
        rs = scenes.camera(W, H)._replace(sh_degree=1)
        sc = scenes.blob_scene(600, 31, 1)
        sc["means3D"][:] = sc["means3D"][0]  # same point -> same depth, same tiles
        sc["means3D"][::3, 0] += 3.0          # a second and third depth class, interleaved
        sc["means3D"][1::3, 0] -= 3.0
        fr = _frame(O, rs, sc)
        assert fr.R > 600
    elif name == "wide":  # 256 tiles: the smallest image that admits a band sort
        W, H = 256, 256
        rs = scenes.camera(W, H)._replace(sh_degree=1)
        sc = scenes.blob_scene(1500, 23, 1)
        fr = _frame(O, rs, sc)
    else:
        W, H = 70, 45
        rs = scenes.camera(W, H, pose_index=21)._replace(sh_degree=1, bg=torch.tensor((0.1, 0.2, 0.3)))
        sc = scenes.blob_scene(1500, 21, 1)
        fr = _frame(O, rs, sc)
        assert int((fr.ranges[:, 1].astype(np.int64) - fr.ranges[:, 0]).max()) > 223
    assert int((fr.ranges[:, 1].astype(np.int64) - fr.ranges[:, 0]).max()) <= 1024 or hint is not None
    _made[name] = (sc["means3D"].shape[0], W, H, rs, sc, fr, hint)
    return _made[name]


def _staged(dev, made, backward, ranks, out_u8=False, **options):
    """One frame through gcr_forward_preprocess + gcr_forward_render under blend_ranks = `ranks` (and `options`); the
    frame's decoded buffers and the mode the host chose for it."""
    from gaussiancity_amd import _native as N, ext
    P, W, H, rs, sc, fr, hint = made
    args = _args(rs, sc, dev)
    (bg, means3D, colors, opacity, scales, rots, scale_modifier, cov, view, proj, tfx, tfy, _, _, sh, degree, campos,
     prefiltered, debug) = args
    cam, keep_cam = ext._camera(dev, bg, view, proj, campos, tfx, tfy, H, W, scale_modifier, degree, prefiltered, debug,
                                backward, False, False, None, out_u8)
    g, keep_g = ext._gaussians(dev, P, means3D, opacity, sh, colors, scales, rots, cov)
    lib, stream = N.lib(), ext._stream(dev)
    byte = dict(dtype=torch.uint8, device=dev)
    geom = torch.empty((lib.gcr_geometry_bytes(P),), **byte)
    img = torch.zeros((lib.gcr_image_bytes(W, H),), **byte)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    info = N.FrameInfo()
    prev = {k: N.set_option(k, v) for k, v in dict(options, blend_ranks=ranks).items()}
    try:
        N.check(lib.gcr_forward_preprocess(C.byref(cam), C.byref(g), geom.data_ptr(), geom.numel(), img.data_ptr(),
                                           img.numel(), radii.data_ptr(), C.byref(info), stream), "gcr_forward_preprocess")
        R = int(info.num_rendered)
        if hint is not None:
            info.max_tile_instances = hint
        out = torch.empty((H, W, 3), **byte) if out_u8 else torch.empty((3, H, W), dtype=torch.float32, device=dev)
        nbytes = lib.gcr_binning_bytes if backward == 1 else lib.gcr_binning_bytes_lean
        binning = torch.zeros((nbytes(R, W, H),), **byte)
        N.check(lib.gcr_forward_render(C.byref(cam), C.byref(g), geom.data_ptr(), geom.numel(), binning.data_ptr(),
                                       binning.numel(), img.data_ptr(), img.numel(), C.byref(info), out.data_ptr(), stream),
                "gcr_forward_render")
        torch.cuda.synchronize()
        mode = N.get_option("last_tile_ids")
        d = G.decode(P, W, H, (R, out, radii, geom, binning, img))  # (while the options still say who wrote the state)
    finally:
        for k, v in prev.items():
            N.set_option(k, v)
    del keep_cam, keep_g
    return dict(d=d, mode=mode, args=args, out=(R, out, radii, geom, binning, img))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("name", ["stack", "ties", "edge"])
def test_frame_is_the_same_bits_with_the_blend_ranking_and_with_the_sort_kernel(oracle_mod, cuda_device, name):
    made = _make(name, oracle_mod)
    P, W, H, rs, sc, fr, hint = made
    on, off = _staged(cuda_device, made, 0, 1), _staged(cuda_device, made, 0, 0)
    assert on["mode"] == 1 and off["mode"] == 0, "the host did not choose the modes this test compares"
    a, b = on["d"], off["d"]
    assert a["R"] == b["R"] == fr.R
    np.testing.assert_array_equal(a["ranges"], b["ranges"])
    n = fr.ranges[:, 1].astype(np.int64) - fr.ranges[:, 0]
    # (an empty tile sits at (e, e), e = the end of the list in front of it; the oracle leaves it at (0, 0))
    np.testing.assert_array_equal(a["ranges"][:, 1].astype(np.int64) - a["ranges"][:, 0], n)
    np.testing.assert_array_equal(a["ranges"][n > 0], fr.ranges[n > 0])
    for k, ref in (("out_color", fr.out_color), ("radii", fr.radii), ("final_T", fr.final_T.ravel()),
                   ("n_contrib", fr.n_contrib.ravel())):
        assert np.array_equal(_bits(a[k]).ravel(), _bits(b[k]).ravel()), k + ": on and off differ"
        assert np.array_equal(_bits(a[k]).ravel(), _bits(ref.astype(a[k].dtype, copy=False)).ravel()), k + ": not the oracle's"
    # the sorted per-tile lists: the ranking blend sorts every list whole (and says so in the lazy-sort states) ...
    np.testing.assert_array_equal(a["point_list"], fr.point_list[:fr.R])
    np.testing.assert_array_equal(a["tile_sorted"].astype(np.int64), n)
    # ... the sort kernel as far as its lazy sort says (whole up to 1024 entries); where both are final they are equal
    G.assert_point_list(b, fr)
    G.assert_point_list(a, fr)


def test_training_frame_ranked_by_the_blend_holds_the_gradient_bar(oracle_mod, cuda_device):
    """gcr_camera.backward == 1 in the "tile ids" mode: the STATE instantiation writes the sorted list, the staged records
    and the block masks at the rank.  Lists of one piece (ranked while staged) and of several (ranked in front of the
    walk); the eight gradient tensors inside the tier test_gpu_parity holds every frame to.  By default a training frame
    keeps the six launches (its blend would grow by more than its sort kernel takes); "sort_in_blend" asks for the mode."""
    from gaussiancity_amd import ext
    made = _make("edge", oracle_mod)
    P, W, H, rs, sc, fr, hint = made
    assert _staged(cuda_device, made, 1, 1)["mode"] == 0
    f = _staged(cuda_device, made, 1, 1, sort_in_blend=1)
    assert f["mode"] == 1
    d = f["d"]
    assert np.array_equal(_bits(d["out_color"]), _bits(fr.out_color))
    np.testing.assert_array_equal(d["point_list"], fr.point_list[:fr.R])
    (bg, means3D, colors, opacity, scales, rots, scale_modifier, cov, view, proj, tfx, tfy, _, _, sh, degree, campos,
     prefiltered, debug) = f["args"]
    R, out, radii, geom, binning, img = f["out"]
    dpix = np.random.default_rng(9).normal(size=(3, H, W)).astype(np.float32)
    grads = ext.rasterize_gaussians_backward(bg, means3D, radii, colors, scales, rots, scale_modifier, cov, view, proj, tfx,
                                             tfy, G.to_dev(dpix, cuda_device), sh, degree, campos, geom, R, binning, img, debug)
    torch.cuda.synchronize()
    names = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot")
    _check_grads(fr.backward(dpix), {k: t.cpu().numpy() for k, t in zip(names, grads)}, list(names))


def test_asynchronous_image_only_and_video_frames_ranked_by_the_blend(oracle_mod, cuda_device):
    from gaussiancity_amd import _native as N, ext
    made = _make("edge", oracle_mod)
    P, W, H, rs, sc, fr, hint = made
    args = _args(rs, sc, cuda_device)
    assert N.get_option("blend_ranks") == 1, "the mode is the default"
    ext._capacity_hint.pop((cuda_device.index, P, W, H), None)
    # the first frame of a key is synchronous and leaves the hints; the second one goes through gcr_forward_async
    for k in range(2):
        t, image = ext.rasterize_gaussians_ticket(*args)[:2]
        assert int(t) == fr.R
        torch.cuda.synchronize()
        assert N.get_option("last_tile_ids") == 1
        assert np.array_equal(_bits(image.cpu().numpy()), _bits(fr.out_color)), "frame %d" % k
    # the image-only frame of GaussianRasterizer.forward under no_grad (no per-pixel state, no list_out)
    image, radii = ext.rasterize_gaussians_frame(*args[:18])
    torch.cuda.synchronize()
    assert N.get_option("last_tile_ids") == 1
    assert np.array_equal(_bits(image.cpu().numpy()), _bits(fr.out_color))
    np.testing.assert_array_equal(radii.cpu().numpy(), fr.radii)
    # uint8 video frames [H,W,3]: (clamp(c, -1, 1) / 2 + 0.5) * 255 in float32, truncated (include/gcr.h, out_u8)
    c = np.clip(fr.out_color, np.float32(-1), np.float32(1)) / np.float32(2) + np.float32(0.5)
    video = np.ascontiguousarray((c * np.float32(255)).astype(np.uint8).transpose(1, 2, 0))
    for backward in (0, N.BACKWARD_IMAGE_ONLY):
        f = _staged(cuda_device, made, backward, 1, out_u8=True)
        assert f["mode"] == 1
        assert np.array_equal(f["out"][1].cpu().numpy(), video)


def test_host_keeps_the_sort_kernel_for_long_lists_band_sorted_frames_and_the_ab_paths(oracle_mod, cuda_device):
    """The mode is for frames whose longest-list hint is at most 1024, whose scatter is not the band-sorted one, and
    neither under force_global_cursor nor under force_radix; everything else takes the six launches (or the radix path).
    A frame in the mode runs in front of each of them, so that a read-back left over from it would show."""
    made = _make("stack", oracle_mod)
    exact = made[:6] + (None,)  # the exact longest list (1100) as the hint
    assert _staged(cuda_device, exact, 0, 1)["mode"] == 0
    wide = _make("wide", oracle_mod)
    for opt, value in (("band_sort_min", 0), ("force_global_cursor", 1), ("force_radix", 1)):
        f = _staged(cuda_device, wide, 0, 1)
        assert f["mode"] == 1 and np.array_equal(_bits(f["d"]["out_color"]), _bits(wide[5].out_color))
        f = _staged(cuda_device, wide, 0, 1, **{opt: value})
        assert f["mode"] == 0, opt
        assert np.array_equal(_bits(f["d"]["out_color"]), _bits(wide[5].out_color)), opt
