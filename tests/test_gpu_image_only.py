"""-m gpu: image-only frames (gcr_camera.backward = GCR_BACKWARD_IMAGE_ONLY, include/gcr.h) through the C ABI with
caller-owned buffers.  Such a frame is an inference frame whose per-pixel state final_T / n_contrib is not written
either: the image and the radii are the same bits, the two regions of the image buffer are left alone, and the
state-only pass (gcr_forward_render with out_color = NULL and backward = 1) writes them -- the oracle's bits -- so that
a backward can follow.  70 x 45 pixels (partial tiles on both edges); one scene whose lists are longer than a chunk of
the blend (223 entries), one whose lists are longer than the lazy sort's first segment (1024) with pixels that walk
beyond it."""
import ctypes as C

import numpy as np
import pytest
import torch

import gpu_util as G
import scenes
from test_gpu_async import _args
from test_gpu_parity import _frame

pytestmark = pytest.mark.gpu

W, H = 70, 45
FILL = 0xA5
SCENES = {
    # name: (P, seed, blob_scene keywords, lists longer than, a pixel walks beyond)
    "lists_over_223": (1500, 21, dict(), 223, 223),
    "lists_over_1024": (6000, 22, dict(smax=8.0, omin=0.002, omax=0.02), 1024, 1024),
}


_made = {}


def _make(name, O):
    """(P, settings, scene, the oracle's frame) of a scene: computed once, shared, never changed."""
    if name not in _made:
        P, seed, kw, longer, deeper = SCENES[name]
        rs = scenes.camera(W, H, pose_index=seed % 24)._replace(sh_degree=2, bg=torch.tensor((0.1, 0.2, 0.3)))
        sc = scenes.blob_scene(P, seed, 2, **kw)
        fr = _frame(O, rs, sc)
        assert int((fr.ranges[:, 1].astype(np.int64) - fr.ranges[:, 0]).max()) > longer and int(fr.n_contrib.max()) > deeper
        _made[name] = (P, rs, sc, fr)
    return _made[name]


@pytest.fixture(params=list(SCENES))
def scene(request, oracle_mod):
    return _make(request.param, oracle_mod)


class _Staged:
    """gcr_forward_preprocess + gcr_forward_render into buffers of the test's own; the image buffer is filled with
    FILL bytes before the frame."""

    def __init__(self, dev, rs, sc, P, backward, flips=False, window=None, out_u8=False):
        from gaussiancity_amd import _native as N, ext
        (bg, means3D, colors, opacity, scales, rots, scale_modifier, cov, view, proj, tfx, tfy, _, _, sh, degree, campos,
         prefiltered, debug) = self.args = _args(rs, sc, dev)
        self.cam, self.keep_cam = ext._camera(dev, bg, view, proj, campos, tfx, tfy, H, W, scale_modifier, degree, prefiltered,
                                              debug, backward, flips, flips, window, out_u8)
        assert self.cam.backward == backward
        self.g, self.keep_g = ext._gaussians(dev, P, means3D, opacity, sh, colors, scales, rots, cov)
        self.lib, self.stream, self.dev, self.P = N.lib(), ext._stream(dev), dev, P
        byte = dict(dtype=torch.uint8, device=dev)
        self.geom = torch.empty((self.lib.gcr_geometry_bytes(P),), **byte)
        self.img = torch.full((self.lib.gcr_image_bytes(W, H),), FILL, **byte)
        self.radii = torch.empty((P,), dtype=torch.int32, device=dev)
        self.info = N.FrameInfo()
        N.check(self.lib.gcr_forward_preprocess(C.byref(self.cam), C.byref(self.g), self.geom.data_ptr(), self.geom.numel(),
                                                self.img.data_ptr(), self.img.numel(), self.radii.data_ptr(),
                                                C.byref(self.info), self.stream), "gcr_forward_preprocess")
        self.R = int(self.info.num_rendered)
        oh, ow = (window[3], window[2]) if window else (H, W)
        self.out = (torch.empty((oh, ow, 3), **byte) if out_u8 else
                    torch.empty((3, oh, ow), dtype=torch.float32, device=dev))
        self.binning = torch.empty((self.lib.gcr_binning_bytes_lean(self.R, W, H),), **byte)
        self.render(self.out)
        self.L = N.get_layout(P, W, H, self.R)

    def render(self, out):
        from gaussiancity_amd import _native as N
        N.check(self.lib.gcr_forward_render(C.byref(self.cam), C.byref(self.g), self.geom.data_ptr(), self.geom.numel(),
                                            self.binning.data_ptr(), self.binning.numel(), self.img.data_ptr(),
                                            self.img.numel(), C.byref(self.info), out.data_ptr() if out is not None else None,
                                            self.stream), "gcr_forward_render")
        torch.cuda.synchronize()

    def state_only_pass(self):
        self.cam.backward = 1
        self.binning = torch.empty((self.lib.gcr_binning_bytes(self.R, W, H),), dtype=torch.uint8, device=self.dev)
        self.render(None)

    def pixel_state(self):
        """(final_T, n_contrib) regions of the image buffer as raw bytes."""
        ib, L = self.img.cpu().numpy(), self.L
        return ib[L.img_final_T:L.img_final_T + 4 * W * H], ib[L.img_n_contrib:L.img_n_contrib + 4 * W * H]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_image_and_radii_are_the_oracles_and_the_pixel_state_is_left_alone(cuda_device, scene):
    from gaussiancity_amd import _native as N
    P, rs, sc, fr = scene
    plain = _Staged(cuda_device, rs, sc, P, 0)
    only = _Staged(cuda_device, rs, sc, P, N.BACKWARD_IMAGE_ONLY)
    assert plain.R == only.R == fr.R
    # (a) image and radii: the oracle's bits, and the bits of the frame rendered with backward = 0
    for f in (plain, only):
        assert _same_bits(f.out.cpu().numpy(), fr.out_color)
        np.testing.assert_array_equal(f.radii.cpu().numpy(), fr.radii)
    # ... whose per-pixel state is there, as ever
    T0, n0 = plain.pixel_state()
    assert _same_bits(T0.view(np.float32), fr.final_T.ravel()) and np.array_equal(n0.view(np.uint32), fr.n_contrib.ravel())
    # (b) the image-only frame wrote neither region
    T1, n1 = only.pixel_state()
    assert (T1 == FILL).all() and (n1 == FILL).all()
    # (c) the state-only pass writes both: the oracle's bits
    only.state_only_pass()
    T2, n2 = only.pixel_state()
    assert _same_bits(T2.view(np.float32), fr.final_T.ravel()) and np.array_equal(n2.view(np.uint32), fr.n_contrib.ravel())


def test_a_backward_after_the_state_only_pass_of_an_image_only_frame(oracle_mod, cuda_device):
    """gcr_backward on the image-only frame's buffers once the state-only pass has run: the oracle's gradients, to the
    bar test_gpu_parity holds every frame to (1e-4 of the largest)."""
    from gaussiancity_amd import _native as N, ext
    from test_gpu_parity import _check_grads
    P, rs, sc, fr = _make("lists_over_223", oracle_mod)
    only = _Staged(cuda_device, rs, sc, P, N.BACKWARD_IMAGE_ONLY)
    only.state_only_pass()
    dpix = np.random.default_rng(9).normal(size=(3, H, W)).astype(np.float32)
    (bg, means3D, colors, opacity, scales, rots, scale_modifier, cov, view, proj, tfx, tfy, _, _, sh, degree, campos,
     prefiltered, debug) = only.args
    grads = ext.rasterize_gaussians_backward(bg, means3D, only.radii, colors, scales, rots, scale_modifier, cov, view, proj,
                                             tfx, tfy, G.to_dev(dpix, cuda_device), sh, degree, campos, only.geom, only.R,
                                             only.binning, only.img, debug)
    torch.cuda.synchronize()
    names = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot")
    _check_grads(fr.backward(dpix), {n: t.cpu().numpy() for n, t in zip(names, grads)},
                 ["dL_dmean2D", "dL_dopacity", "dL_dmean3D", "dL_dsh", "dL_dscale", "dL_drot"])


def test_window_of_the_mirrored_image_and_video_bytes(cuda_device, scene):
    from gaussiancity_amd import _native as N
    P, rs, sc, fr = scene
    window = (9, 6, 40, 30)  # x, y, w, h of the mirrored image: cuts through tiles on every side
    want = np.ascontiguousarray(fr.out_color[:, ::-1, ::-1][:, 6:36, 9:49])
    plain = _Staged(cuda_device, rs, sc, P, 0, flips=True, window=window)
    only = _Staged(cuda_device, rs, sc, P, N.BACKWARD_IMAGE_ONLY, flips=True, window=window)
    for f in (plain, only):
        assert _same_bits(f.out.cpu().numpy(), want)
        np.testing.assert_array_equal(f.radii.cpu().numpy(), fr.radii)
    T1, n1 = only.pixel_state()
    assert (T1 == FILL).all() and (n1 == FILL).all()
    # uint8 video frames [H,W,3]: (clamp(c, -1, 1) / 2 + 0.5) * 255 in float32, truncated (include/gcr.h, out_u8)
    c = np.clip(fr.out_color, np.float32(-1), np.float32(1)) / np.float32(2) + np.float32(0.5)
    video = np.ascontiguousarray((c * np.float32(255)).astype(np.uint8).transpose(1, 2, 0))
    plain = _Staged(cuda_device, rs, sc, P, 0, out_u8=True)
    only = _Staged(cuda_device, rs, sc, P, N.BACKWARD_IMAGE_ONLY, out_u8=True)
    for f in (plain, only):
        assert _same_bits(f.out.cpu().numpy(), video)
    T1, n1 = only.pixel_state()
    assert (T1 == FILL).all() and (n1 == FILL).all()


def test_gaussian_rasterizer_under_no_grad_renders_image_only_frames(cuda_device, scene, monkeypatch):
    """(d) GaussianRasterizer.forward without a gradient in sight is the image-only frame: the same image and radii,
    several frames in a row (the first of a key takes the synchronous path, the later ones the asynchronous one)."""
    from gaussiancity_amd import _native as N, ext
    from gaussiancity_amd.rasterizer import GaussianRasterizer
    P, rs, sc, fr = scene
    seen = []
    forward = ext._forward

    def spy(L, device, cam, g, P_, H_, W_, mode):
        seen.append((int(cam.backward), mode))
        return forward(L, device, cam, g, P_, H_, W_, mode)
    monkeypatch.setattr(ext, "_forward", spy)
    dev = cuda_device
    rs_dev = rs._replace(bg=rs.bg.to(dev), view_matrix=rs.view_matrix.to(dev), proj_matrix=rs.proj_matrix.to(dev),
                         campos=rs.campos.to(dev))
    t = {k: G.to_dev(sc[k], dev) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    ras = GaussianRasterizer(rs_dev)
    with torch.no_grad():
        frames = [ras(t["means3D"], torch.zeros_like(t["means3D"]), t["opacities"], shs=t["shs"], scales=t["scales"],
                      rotations=t["rotations"]) for _ in range(4)]
    torch.cuda.synchronize()
    assert seen == [(N.BACKWARD_IMAGE_ONLY, ext._IMAGE)] * 4
    for color, radii in frames:
        assert _same_bits(color.cpu().numpy(), fr.out_color)
        np.testing.assert_array_equal(radii.cpu().numpy(), fr.radii)
    # a frame that hands its buffers out keeps its per-pixel state
    seen.clear()
    args, out = G.run_forward(rs, sc, dev, for_backward=False)
    assert seen == [(0, ext._INT)]
    d = G.decode(P, W, H, out)
    np.testing.assert_array_equal(d["n_contrib"], fr.n_contrib.ravel())
    assert _same_bits(d["final_T"], fr.final_T.ravel())
