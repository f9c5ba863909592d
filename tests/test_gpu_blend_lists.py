"""-m gpu: the forward blend's two-level list build and its chunk sort in registers (gcr_blend.hip "two-level list
build", gcr_sort.h gcr_sort_merge).  A wave first gathers the slots that reach its 8x8 quadrant at all (its dense list)
and compacts only those into its eight sub-row lists; the one-chunk "tile ids" path sorts every 64-key chunk in
registers and a thread stages the entry whose key its lane holds afterwards.  Neither changes a bit of a frame: image,
final_T, n_contrib, num_rendered and the sorted per-tile lists are the oracle's, with option "blend_ranks" on and off.

Scenes (64 x 48 pixels = 12 tiles and at most about 1 500 Gaussians; "edge" is 70 x 45).  A "stack" is a number of small
Gaussians on ONE pixel of a tile, a few pixels wide: on pixel (4, 4) it stays inside the tile's first quadrant, so that
quadrant's wave gets a dense list of the whole chunk and the three other waves an empty one.
  * "quad_a", "quad_b": one-quadrant stacks of 0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 222 and 223 entries -- every
    count around the 64-entry groups of both levels and the longest chunk;
    "quad_b" also holds the mixed tiles: 223 entries of which exactly 64 (65 in another tile) reach the first quadrant and
    the others the fourth, and a tile of 220 whose 20 entries of the second quadrant are the deepest ones (slots 200..219:
    the last source group only);
  * "full": 223 Gaussians wider than a tile on the centre of the image: every entry reaches all 32 blocks of the tile,
    the dense lists are the whole chunk (four level-2 groups);
  * "ties": stacks of 64 at ONE depth (the index decides), of 65, 128 and 129 in two alternating depth classes, and lists
    of 224 and 600 (ranked in front of the walk, walked in chunks: the paths the list build shares);
  * "edge": 70 x 45, partial tiles on both edges, lists beyond a chunk (1 400 Gaussians: a size of its own, so that the
    frames of this file share no (P, W, H) hint key with the asynchronous frames of tests/test_gpu_blend_ranks.py).
What a scene promises (list lengths, untouched quadrants, fully covered tiles) is asserted on the oracle's frame alone."""
import numpy as np
import pytest
import torch

import gpu_util as G
import scenes
from test_gpu_blend_ranks import _bits, _staged
from test_gpu_parity import _check_grads, _frame

pytestmark = pytest.mark.gpu

W0, H0 = 64, 48
QUAD = (4, 4)      # pixel of a tile: the middle of its first quadrant (wave 0)
QUAD2 = (12, 4)    # ... of its second (wave 1)
QUAD4 = (12, 12)   # ... of its fourth (wave 3)


def _alternating(j):
    return 60.0 + 2.0 * (j % 2)


def _nine(j):
    return 60.0 + 0.25 * (j % 9)


def _scene(rs, W, H, stacks, seed, scale=0.02, opacity=(0.003, 0.03)):
    """`stacks`: (tile, (px, py) inside the tile, count, depth of entry j).  Index order unrelated to tile and depth.
    Returns the scene and, per Gaussian, the number of its stack."""
    rng = np.random.default_rng(seed)
    gx = (W + 15) // 16
    inv = np.linalg.inv(rs.view_matrix.cpu().numpy().astype(np.float64))  # row vectors: p_view = [p, 1] @ view
    pts, label = [], []
    for k, (t, (ox, oy), n, depth) in enumerate(stacks):
        px, py = (t % gx) * 16 + float(ox), (t // gx) * 16 + float(oy)
        ndc_x, ndc_y = (2 * px + 1) / W - 1, (2 * py + 1) / H - 1
        for j in range(n):
            z = depth(j)
            label.append(k)
            pts.append((np.array([-ndc_x * rs.tanfovx * z, -ndc_y * rs.tanfovy * z, z, 1.0]) @ inv)[:3])  # (the view looks down -x, -y)
    P = len(pts)
    order = rng.permutation(P)
    xyz = np.asarray(pts, np.float32).reshape(P, 3)[order]
    shs = np.zeros((P, 4, 3), np.float32)
    shs[:, 0] = rng.normal(0.3, 0.8, (P, 3))
    rot = np.zeros((P, 4), np.float32)
    rot[:, 0] = 1.0
    sc = dict(means3D=xyz, scales=np.full((P, 3), scale, np.float32), rotations=rot,
              opacities=rng.uniform(opacity[0], opacity[1], (P, 1)).astype(np.float32),
              colors_precomp=rng.uniform(-1, 1, (P, 3)).astype(np.float32), shs=shs, sh_degree=1)
    return sc, np.asarray(label, np.int64)[order]


def _tile_px(a, W, H, t):
    """The 16 x 16 pixels of tile t of a per-pixel array (image 64 x 48: no partial tiles)."""
    gx = W // 16
    return np.asarray(a).reshape(H, W)[(t // gx) * 16:(t // gx) * 16 + 16, (t % gx) * 16:(t % gx) * 16 + 16]


QUAD_A = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192)
QUAD_B = (193, 222, 223)
_made = {}


def _make(name, O):
    """(P, W, H, settings, scene, the oracle's frame, None): computed once, shared, never changed."""
    if name in _made:
        return _made[name]
    W, H = W0, H0
    rs = scenes.camera(W, H)._replace(sh_degree=1, bg=torch.tensor((0.1, 0.2, 0.3)))
    if name in ("quad_a", "quad_b"):
        lengths = QUAD_A if name == "quad_a" else QUAD_B
        stacks = [(t, QUAD, n, _nine) for t, n in enumerate(lengths)]
        want = {t: n for t, n in enumerate(lengths)}
        if name == "quad_b":
            stacks += [(3, QUAD, 64, _nine), (3, QUAD4, 159, _nine), (4, QUAD, 65, _nine), (4, QUAD4, 158, _nine),
                       (5, QUAD, 200, _nine), (5, QUAD2, 20, lambda j: 70.0 + 0.25 * (j % 3))]
            want.update({3: 223, 4: 223, 5: 220})
        sc, label = _scene(rs, W, H, stacks, 5)
        fr = _frame(O, rs, sc)
        n = fr.ranges[:, 1].astype(np.int64) - fr.ranges[:, 0]
        for t in range(12):
            assert n[t] == want.get(t, 0), (t, int(n[t]))
        for t, length in enumerate(lengths):  # one-quadrant stacks: the other three quadrants see nothing
            nc = _tile_px(fr.n_contrib, W, H, t)
            assert nc[8:, :].max() == 0 and nc[:8, 8:].max() == 0
            assert nc[:8, :8].max() == length  # ... and the first one walks its list to the end
        if name == "quad_b":
            for t, k, st in ((3, 64, 3), (4, 65, 5)):  # exactly k entries in the first quadrant, the others in the fourth
                nc = _tile_px(fr.n_contrib, W, H, t)
                of = label[fr.point_list[fr.ranges[t, 0]:fr.ranges[t, 1]]]  # the stack of every list entry
                assert int((of == st).sum()) == k and int((of == st + 1).sum()) == 223 - k
                assert nc[:8, 8:].max() == 0 and nc[8:, :8].max() == 0
                # a pixel's last contributor is an entry of its own quadrant's stack, and both stacks are walked to their end
                q1, q4 = nc[:8, :8], nc[8:, 8:]
                assert (of[q1[q1 > 0] - 1] == st).all() and (of[q4[q4 > 0] - 1] == st + 1).all()
                assert q1.max() == np.flatnonzero(of == st)[-1] + 1 and q4.max() == np.flatnonzero(of == st + 1)[-1] + 1
            nc = _tile_px(fr.n_contrib, W, H, 5)  # the second quadrant's entries are the tile's last twenty
            assert nc[:8, 8:].max() == 220 and nc[:8, 8:][nc[:8, 8:] > 0].min() > 200 and nc[:8, :8].max() == 200
            assert nc[8:, :].max() == 0
    elif name == "full":
        sc, _ = _scene(rs, W, H, [(5, (8, 8), 223, _nine)], 6, scale=5.0, opacity=(0.02, 0.03))
        fr = _frame(O, rs, sc)
        n = fr.ranges[:, 1].astype(np.int64) - fr.ranges[:, 0]
        assert n.min() == 223 and n.max() == 223  # (wide enough to reach every tile of the image)
        # every pixel of the tile ends at the list's last entry: every block's list holds it, four groups deep
        assert _tile_px(fr.n_contrib, W, H, 5).min() == 223
    elif name == "ties":
        stacks = [(0, QUAD, 64, lambda j: 60.0), (1, QUAD, 65, _alternating), (2, QUAD, 128, _alternating),
                  (3, QUAD, 129, _alternating), (4, QUAD, 224, _nine), (5, QUAD, 600, _nine)]
        sc, _ = _scene(rs, W, H, stacks, 7)
        fr = _frame(O, rs, sc)
        n = fr.ranges[:, 1].astype(np.int64) - fr.ranges[:, 0]
        assert list(n[:6]) == [64, 65, 128, 129, 224, 600] and n[6:].max() == 0
        d = fr.depths[fr.point_list[fr.ranges[0, 0]:fr.ranges[0, 1]]]
        assert np.unique(d).size == 1  # one depth: the index alone decides
        for t in (1, 2, 3):
            assert np.unique(fr.depths[fr.point_list[fr.ranges[t, 0]:fr.ranges[t, 1]]]).size == 2
        assert int(_tile_px(fr.n_contrib, W, H, 5).max()) > 446  # the walk gets into the third chunk of the 600
    else:
        W, H = 70, 45
        rs = scenes.camera(W, H, pose_index=21)._replace(sh_degree=1, bg=torch.tensor((0.1, 0.2, 0.3)))
        sc = scenes.blob_scene(1400, 22, 1)
        fr = _frame(O, rs, sc)
        assert int((fr.ranges[:, 1].astype(np.int64) - fr.ranges[:, 0]).max()) > 223
    assert int((fr.ranges[:, 1].astype(np.int64) - fr.ranges[:, 0]).max()) <= 1024
    _made[name] = (sc["means3D"].shape[0], W, H, rs, sc, fr, None)
    return _made[name]


def _video(fr):
    c = np.clip(fr.out_color, np.float32(-1), np.float32(1)) / np.float32(2) + np.float32(0.5)
    return np.ascontiguousarray((c * np.float32(255)).astype(np.uint8).transpose(1, 2, 0))


@pytest.mark.parametrize("name", ["quad_a", "quad_b", "full", "ties", "edge"])
def test_frames_are_the_oracles_bits_with_two_level_lists(oracle_mod, cuda_device, name):
    from gaussiancity_amd import _native as N
    made = _make(name, oracle_mod)
    P, W, H, rs, sc, fr, hint = made
    n = fr.ranges[:, 1].astype(np.int64) - fr.ranges[:, 0]
    # frames that keep their state: "tile ids" (the blend ranks: chunk sort in registers) and the sort kernel
    for ranks in (1, 0):
        f = _staged(cuda_device, made, 0, ranks)
        assert f["mode"] == ranks, "the host did not choose the mode this test asks for"
        d = f["d"]
        assert d["R"] == fr.R
        np.testing.assert_array_equal(d["ranges"][:, 1].astype(np.int64) - d["ranges"][:, 0], n)
        np.testing.assert_array_equal(d["ranges"][n > 0], fr.ranges[n > 0])
        for k, ref in (("out_color", fr.out_color), ("final_T", fr.final_T.ravel()), ("n_contrib", fr.n_contrib.ravel())):
            assert np.array_equal(_bits(d[k]).ravel(), _bits(ref.astype(d[k].dtype, copy=False)).ravel()), \
                "%s: not the oracle's (blend_ranks = %d)" % (k, ranks)
        if ranks:  # the ranking blend sorts every list whole
            np.testing.assert_array_equal(d["point_list"], fr.point_list[:fr.R])
            np.testing.assert_array_equal(d["tile_sorted"].astype(np.int64), n)
        G.assert_point_list(d, fr)
    # image-only frames (no per-pixel state, no list_out) and uint8 video frames, both modes
    video = _video(fr)
    for ranks in (1, 0):
        f = _staged(cuda_device, made, N.BACKWARD_IMAGE_ONLY, ranks)
        assert f["mode"] == ranks
        assert np.array_equal(_bits(f["d"]["out_color"]), _bits(fr.out_color)), "image-only, blend_ranks = %d" % ranks
        for backward in (0, N.BACKWARD_IMAGE_ONLY):
            f = _staged(cuda_device, made, backward, ranks, out_u8=True)
            assert f["mode"] == ranks
            assert np.array_equal(f["out"][1].cpu().numpy(), video), "uint8, backward = %d, blend_ranks = %d" % (backward, ranks)


@pytest.mark.parametrize("name", ["quad_b", "edge"])
def test_training_frame_sorted_in_the_blend_holds_the_gradient_bar(oracle_mod, cuda_device, name):
    """gcr_camera.backward == 1 through "sort_in_blend": the STATE instantiation builds the same lists and leaves the
    sorted list, the staged records and the block masks at the rank of the key a thread holds AFTER the chunk sort."""
    from gaussiancity_amd import ext
    made = _make(name, oracle_mod)
    P, W, H, rs, sc, fr, hint = made
    f = _staged(cuda_device, made, 1, 1, sort_in_blend=1)
    assert f["mode"] == 1
    d = f["d"]
    assert np.array_equal(_bits(d["out_color"]), _bits(fr.out_color))
    assert np.array_equal(_bits(d["final_T"]), _bits(fr.final_T.ravel()))
    np.testing.assert_array_equal(d["n_contrib"], fr.n_contrib.ravel())
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
