#!/usr/bin/env python
"""Generates tests/golden/image_loss.npz with the REFERENCE's own losses/gan.py and models/discriminator.py, imported by
path on the CPU (both need only torch), and with the lines of core/train.py:285 as torch runs them.  Run in the build
container only (the reference does not exist on the GPU box):

    python tests/golden/make_image_loss_golden.py <reference root>

The fixture holds data only: per case the float32 inputs, and the outputs and gradients of upstream's code run on them in
float32 (`*32`) and on their float64 casts (`*64`).

  gan/<shape>/<form>/<w|nw>   GANLoss in its three call forms -- dis_real (t_real=True, dis_update=True), dis_fake (False,
                              True), gen_real (True, False) -- at pred shapes (2, 9, 7, 5) and (1, 9, 16, 16), with and
                              without a weight: loss and the gradient of pred
  gan_list                    the list form: [[other, x0], x1] at (2, 9, 7, 5), dis_real with a weight
  interp/<HxW>_<hxw>          Discriminator._smooth_interp on a one-hot map times a binary mask with a fully masked
                              rectangle: 29 x 23 -> 7 x 5 and 64 x 64 -> 16 x 16
  l1                          L1Loss()(fake * msk, rgb * msk) at (1, 3, 16, 16): loss and both gradients
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import image_loss_ref as R  # noqa: E402

FORMS = {"dis_real": (True, True), "dis_fake": (False, True), "gen_real": (True, False)}
GAN_SHAPES = [(2, 9, 7, 5), (1, 9, 16, 16)]
INTERP = [(2, 8, (29, 23), (7, 5)), (1, 8, (64, 64), (16, 16))]


def load(root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gan_run(crit, pred, label, weight, form, dtype):
    t_real, dis_update = FORMS[form]
    p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
    x = {"pred": p, "label": torch.from_numpy(label).to(dtype)}
    w = None if weight is None else torch.from_numpy(weight).to(dtype)
    loss = crit(x, t_real, w, dis_update=dis_update)
    loss.backward()
    return loss.detach().numpy(), p.grad.numpy()


def main(root):
    G = load(root, "losses/gan.py", "ref_losses_gan")
    D = load(root, "models/discriminator.py", "ref_models_discriminator")
    crit = G.GANLoss()
    out = {}
    for shape in GAN_SHAPES:
        pred, label, weight = R.gan_inputs(shape, seed=1)
        key = "gan/%s" % "x".join(str(v) for v in shape)
        out[key + "/pred"], out[key + "/label"], out[key + "/weight"] = pred, label, weight
        for form in FORMS:
            for wname, w in (("w", weight), ("nw", None)):
                for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
                    loss, dpred = gan_run(crit, pred, label, w, form, dtype)
                    out["%s/%s/%s/loss%s" % (key, form, wname, tag)] = loss
                    out["%s/%s/%s/dpred%s" % (key, form, wname, tag)] = dpred
    # the list form
    shape = GAN_SHAPES[0]
    ins = [R.gan_inputs(shape, seed=s) for s in (2, 3)]
    weight = ins[0][2]
    out["gan_list/weight"] = weight
    for i, (pred, label, _) in enumerate(ins):
        out["gan_list/pred%d" % i], out["gan_list/label%d" % i] = pred, label
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        ps = [torch.from_numpy(p).to(dtype).requires_grad_(True) for p, _, _ in ins]
        xs = [{"pred": p, "label": torch.from_numpy(l).to(dtype)} for p, (_, l, _) in zip(ps, ins)]
        loss = crit([[xs[1], xs[0]], xs[1]], True, torch.from_numpy(weight).to(dtype), dis_update=True)
        loss.sum().backward()
        out["gan_list/loss" + tag] = loss.detach().numpy()
        for i, p in enumerate(ps):
            out["gan_list/dpred%d_%s" % (i, tag)] = p.grad.numpy()
    # _smooth_interp
    for b, c, (H, W), (h, w) in INTERP:
        seg, mask = R.one_hot_seg(b, c, H, W, seed=4)
        key = "interp/%dx%d_%dx%d" % (H, W, h, w)
        out[key + "/seg"], out[key + "/mask"] = seg.astype(np.uint8), mask.astype(np.uint8)
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            x = torch.from_numpy(seg).to(dtype) * torch.from_numpy(mask).to(dtype)
            out[key + "/out" + tag] = D.Discriminator._smooth_interp(x, (h, w)).numpy().astype(np.uint8)
    # core/train.py:285
    a, b = R.images((1, 3, 16, 16), seed=5)
    msk = R.make_mask("random30", 1, 16, 16, seed=5)
    out["l1/fake"], out["l1/rgb"], out["l1/msk"] = a, b, msk
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        fake = torch.from_numpy(a).to(dtype).requires_grad_(True)
        rgb = torch.from_numpy(b).to(dtype).requires_grad_(True)
        m = torch.from_numpy(msk).to(dtype)
        loss = torch.nn.L1Loss()(fake * m, rgb * m)
        loss.backward()
        out["l1/loss" + tag], out["l1/dfake" + tag], out["l1/drgb" + tag] = loss.detach().numpy(), fake.grad.numpy(), rgb.grad.numpy()
    path = os.path.join(HERE, "image_loss.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))
    for k in sorted(out):
        if k.endswith("loss32"):
            l32, l64 = float(out[k].reshape(-1)[0]), float(out[k[:-2] + "64"].reshape(-1)[0])
            print("  %-40s loss64 %.9g  err32 %.3g" % (k[:-6], l64, abs(l32 - l64)))


if __name__ == "__main__":
    main(sys.argv[1])
