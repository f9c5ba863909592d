"""-m gpu: the image-loss kernels (gaussiancity_amd.image_loss -> include/gcv.h K20-K22) against the float64 restatement of
tests/image_loss_ref.py.

Loss scalars: |loss - loss64| <= 1e-5 T, T the sum of the absolute terms (image_loss_ref.check_loss).  Gradient elements:
|got - ref64| <= 4 E + 2^-22 |ref64|, E the largest error of torch's own float32 lines (image_loss.torch_*) on that tensor,
run on the device in the same test (image_loss_ref.check_grad, which prints got / E).  Label maps: bit for bit against
torch's lines on the device and against the restatement, on one-hot maps times binary masks, whose window sums are exact in
any order."""
import functools

import numpy as np
import pytest
import torch

import image_loss_ref as R
from gaussiancity_amd import image_loss as IL

pytestmark = pytest.mark.gpu


def _dev(a, device, grad=False):
    return None if a is None else torch.from_numpy(np.array(a)).to(device).requires_grad_(grad)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _l1_case(shape, mask):
    """(a, b, mask, loss64, T, da64, db64): computed once, shared, never changed."""
    a, b = R.images(shape)
    m = R.make_mask(mask, shape[0], shape[2], shape[3])
    out = (a, b, m) + R.l1_64(a, b, m)
    for v in out:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _gan_case(shape, real, weighted, scale=3.0, labels="onehot"):
    pred, label, weight = R.gan_inputs(shape, scale=scale, labels=labels)
    w = weight if weighted else None
    out = (pred, label, w) + R.gan64(pred, label, w, real)
    for v in out:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _torch_grads(fn, *leaves):
    """torch's own float32 lines on the device: (loss, the leaves' gradients)."""
    loss = fn()
    loss.backward()
    return loss, [t.grad for t in leaves]


# ---- K20 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.L1_SHAPES + [R.L1_WIDE_SHAPE], ids=str)
def test_l1_against_float64(cuda_device, shape):
    masks = ("none",) if shape == R.L1_WIDE_SHAPE else R.L1_MASKS
    before = IL.stats()
    for name in masks:
        a, b, m, loss64, T, da64, db64 = _l1_case(shape, name)
        what = "l1 %s %s" % (shape, name)
        da_, db_, dm = _dev(a, cuda_device, True), _dev(b, cuda_device, True), _dev(m, cuda_device)
        keep = [t.detach().clone() for t in (da_, db_)] + ([] if dm is None else [dm.clone()])
        loss = IL.l1(da_, db_, dm)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
        loss.backward()
        R.check_loss(loss.item(), loss64, T, what)
        ta, tb = _dev(a, cuda_device, True), _dev(b, cuda_device, True)
        _torch_grads(lambda: IL.torch_l1(ta, tb, dm), ta, tb)
        R.check_grad(da_.grad.cpu().numpy(), da64, ta.grad.cpu().numpy(), what + " da")
        R.check_grad(db_.grad.cpu().numpy(), db64, tb.grad.cpu().numpy(), what + " db")
        assert torch.equal(_bits(db_.grad), _bits(-da_.grad))
        if name == "zeros":
            assert loss.item() == 0.0 and not bool(da_.grad.any()) and not bool(db_.grad.any())
        now = [da_.detach(), db_.detach()] + ([] if dm is None else [dm])
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(now, keep)), what + ": an input was written"
    after = IL.stats()
    assert after["native_calls"] == before["native_calls"] + len(masks) and after["fallback_calls"] == before["fallback_calls"]


def test_l1_strides_and_gradient_subsets(cuda_device):
    shape = (2, 3, 33, 65)
    a, b, m, loss64, T, da64, db64 = _l1_case(shape, "soft")
    dm = _dev(m, cuda_device)
    want = IL.l1(_dev(a, cuda_device), _dev(b, cuda_device), dm)
    # a strided view: row stride 2W + 3, channel stride (H + 5)(2W + 3), a batch stride beyond that
    wide = torch.zeros((2, 4, 33 + 5, 2 * 65 + 3), device=cuda_device)
    view = wide[:, 1:4, 2:35, 3:68]
    view.copy_(_dev(a, cuda_device))
    assert view.stride(3) == 1 and not view.is_contiguous()
    keep = wide.clone()
    leaf_b = _dev(b, cuda_device, True)
    loss = IL.l1(view, leaf_b, dm)
    assert torch.equal(_bits(loss), _bits(want))
    loss.backward()
    assert torch.equal(_bits(wide), _bits(keep))
    # pixel stride 2 (a contiguous copy inside), channels last, an expanded mask (batch stride 0)
    odd = torch.zeros((2, 3, 33, 130), device=cuda_device)[..., ::2]
    odd.copy_(_dev(a, cuda_device))
    assert torch.equal(_bits(IL.l1(odd, _dev(b, cuda_device), dm)), _bits(want))
    cl = _dev(a, cuda_device).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert torch.equal(_bits(IL.l1(cl, _dev(b, cuda_device), dm)), _bits(want))
    one = dm[:1].expand(2, 1, 33, 65)
    assert torch.equal(_bits(IL.l1(_dev(a, cuda_device), _dev(b, cuda_device), one)),
                       _bits(IL.l1(_dev(a, cuda_device), _dev(b, cuda_device), one.contiguous())))
    # only b requires grad (above), only a, both: the same bits wherever a gradient is asked for
    la, lb = _dev(a, cuda_device, True), _dev(b, cuda_device, True)
    IL.l1(la, lb, dm).backward()
    only_a = _dev(a, cuda_device, True)
    fixed_b = _dev(b, cuda_device)
    IL.l1(only_a, fixed_b, dm).backward()
    assert fixed_b.grad is None and torch.equal(_bits(only_a.grad), _bits(la.grad))
    assert torch.equal(_bits(leaf_b.grad), _bits(lb.grad))
    ta, tb = _dev(a, cuda_device, True), _dev(b, cuda_device, True)
    _torch_grads(lambda: IL.torch_l1(ta, tb, dm), ta, tb)
    R.check_grad(la.grad.cpu().numpy(), da64, ta.grad.cpu().numpy(), "l1 strided da")
    R.check_grad(lb.grad.cpu().numpy(), db64, tb.grad.cpu().numpy(), "l1 strided db")
    # an incoming gradient other than 1, read on the device
    lc = _dev(a, cuda_device, True)
    (IL.l1(lc, fixed_b, dm) * 3.0).backward()
    R.check_grad(lc.grad.cpu().numpy(), 3.0 * da64, 3.0 * ta.grad.cpu().numpy(), "l1 g = 3 da")
    no_grad = IL.l1(_dev(a, cuda_device), fixed_b, dm)
    assert not no_grad.requires_grad


# ---- K21 ---------------------------------------------------------------------------------------------------------------
def _gan_check(cuda_device, pred, label, w, real, loss64, T, d64, what):
    p, dl, dw = _dev(pred, cuda_device, True), _dev(label, cuda_device), _dev(w, cuda_device)
    keep = [p.detach().clone(), dl.clone()] + ([] if dw is None else [dw.clone()])
    loss = IL.gan_loss(p, dl, dw, real=real)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    loss.backward()
    R.check_loss(loss.item(), loss64, T, what)
    tp = _dev(pred, cuda_device, True)
    _torch_grads(lambda: IL.torch_gan_loss(tp, dl, dw, real), tp)
    R.check_grad(p.grad.cpu().numpy(), d64, tp.grad.cpu().numpy(), what + " dpred")
    assert tuple(p.grad.shape) == tuple(pred.shape) and not bool(p.grad[:, 0].any()), what + ": channel 0 of dpred is not exactly zero"
    now = [p.detach(), dl] + ([] if dw is None else [dw])
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(now, keep)), what + ": an input was written"


@pytest.mark.parametrize("shape", R.GAN_SHAPES, ids=str)
@pytest.mark.parametrize("real", [True, False], ids=["real", "fake"])
def test_gan_loss_against_float64(cuda_device, shape, real):
    before = IL.stats()
    n = 0
    for weighted in (False, True):
        for labels in ("onehot", "soft"):
            pred, label, w, loss64, T, d64 = _gan_case(shape, real, weighted, labels=labels)
            _gan_check(cuda_device, pred, label, w, real, loss64, T, d64,
                       "gan %s %s %s %s" % (shape, "real" if real else "fake", labels, "w" if weighted else "nw"))
            n += 1
    after = IL.stats()
    assert after["native_calls"] == before["native_calls"] + n and after["fallback_calls"] == before["fallback_calls"]


@pytest.mark.parametrize("real", [True, False], ids=["real", "fake"])
def test_gan_loss_large_logits(cuda_device, real):
    """Logits scaled by 50 (up to about +-200): exp overflows float32 unless the pixel's maximum is subtracted."""
    pred, label, w, loss64, T, d64 = _gan_case((2, 9, 7, 5), real, True, scale=50.0)
    assert np.abs(pred).max() > 100
    _gan_check(cuda_device, pred, label, w, real, loss64, T, d64, "gan x50 %s" % ("real" if real else "fake"))
    pred = np.where(np.arange(9)[None, :, None, None] % 2 == 0, 80.0, -80.0).astype(np.float32) * np.ones((2, 9, 7, 5), np.float32)
    _gan_check(cuda_device, pred, label, w, real, *R.gan64(pred, label, w, real), "gan +-80 %s" % ("real" if real else "fake"))


def test_gan_loss_on_labels_from_label_map(cuda_device):
    seg, mask = R.one_hot_seg(1, 8, 64, 64)
    dseg, dmask = _dev(seg, cuda_device), _dev(mask, cuda_device)
    label = IL.label_map(dseg, (16, 16), dmask)
    hole = label[:, 0, 4:12, 4:12]
    assert bool(hole.all()), "a window that is masked out entirely must give channel 0"
    pred, _, weight = R.gan_inputs((1, 9, 16, 16), seed=3)
    lab = label.cpu().numpy()
    for real in (True, False):
        loss64, T, d64 = R.gan64(pred, lab, weight, real)
        _gan_check(cuda_device, pred, lab, weight, real, loss64, T, d64, "gan on label_map labels %s" % ("real" if real else "fake"))
    # the pixels of channel 0 add nothing in the real mode: their gradient is zero in every channel
    p = _dev(pred, cuda_device, True)
    IL.gan_loss(p, label, None, real=True).backward()
    assert not bool(p.grad[:, :, 4:12, 4:12].any())


def test_gan_loss_strides(cuda_device):
    pred, label, w, *_ = _gan_case((3, 5, 16, 16), True, True)
    want = IL.gan_loss(_dev(pred, cuda_device), _dev(label, cuda_device), _dev(w, cuda_device))
    wide = torch.zeros((3, 7, 20, 37), device=cuda_device)
    view = wide[:, 1:6, 2:18, 5:21]
    view.copy_(_dev(pred, cuda_device))
    lab_cl = _dev(label, cuda_device).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)       # pixel stride 4: copied
    leaf = view.detach().requires_grad_(True)
    loss = IL.gan_loss(leaf, lab_cl, _dev(w, cuda_device))
    assert torch.equal(_bits(loss), _bits(want))
    loss.backward()
    p = _dev(pred, cuda_device, True)
    IL.gan_loss(p, _dev(label, cuda_device), _dev(w, cuda_device)).backward()
    assert leaf.grad.shape == leaf.shape and torch.equal(_bits(leaf.grad), _bits(p.grad))


# ---- K22 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", R.LABEL_SIZES, ids=str)
@pytest.mark.parametrize("c", R.LABEL_CLASSES)
def test_label_map_bit_for_bit(cuda_device, src, dst, c):
    b = 1 if src[0] > 100 else 2
    seg, mask = R.one_hot_seg(b, c, *src)
    dseg, dmask = _dev(seg, cuda_device), _dev(mask, cuda_device)
    before = IL.stats()
    for m, dm in ((None, None), (mask, dmask)):
        keep = dseg.clone()
        got = IL.label_map(dseg, dst, dm)
        assert got.dtype == torch.float32 and tuple(got.shape) == (b, c) + tuple(dst) and got.is_contiguous() and not got.requires_grad
        assert torch.equal(_bits(got), _bits(IL.torch_label_map(dseg, dst, dm))), "differs from torch's lines on the device"
        assert np.array_equal(got.cpu().numpy(), R.label_map64_fast(seg, dst, m)), "differs from the restatement"
        assert torch.equal(_bits(dseg), _bits(keep))
        assert torch.equal(_bits(got), _bits(IL.label_map(dseg, dst, dm)))
    after = IL.stats()
    assert after["native_calls"] == before["native_calls"] + 4 and after["fallback_calls"] == before["fallback_calls"]


def test_label_map_tie_strides_and_refusals(cuda_device):
    seg = np.zeros((1, 4, 4, 4), np.float32)
    seg[0, 3, :2], seg[0, 1, 2:] = 1.0, 1.0          # channels 3 and 1 cover half of the one window each
    got = IL.label_map(_dev(seg, cuda_device), (1, 1))
    assert got.reshape(-1).tolist() == [0.0, 1.0, 0.0, 0.0]
    seg, mask = R.one_hot_seg(2, 8, 33, 65)
    dseg, dmask = _dev(seg, cuda_device), _dev(mask, cuda_device)
    want = IL.label_map(dseg, (8, 16), dmask)
    wide = torch.zeros((2, 9, 40, 70), device=cuda_device)
    view = wide[:, 1:, 3:36, 2:67]
    view.copy_(dseg)
    assert torch.equal(_bits(IL.label_map(view, (8, 16), dmask)), _bits(want))
    assert torch.equal(_bits(IL.label_map(dseg, (8, 16), dmask[:1].expand(2, 1, 33, 65))), _bits(IL.label_map(dseg, (8, 16), dmask[:1].repeat(2, 1, 1, 1))))
    with pytest.raises(RuntimeError):
        IL.label_map(dseg.clone().requires_grad_(True), (8, 16))
    before = IL.stats()["fallback_calls"]
    assert tuple(IL.label_map(dseg, (66, 130)).shape) == (2, 8, 66, 130)       # larger than the source: torch's lines
    assert IL.stats()["fallback_calls"] == before + 1


# ---- golden, repeatability, bookkeeping ------------------------------------------------------------------------------------
def test_golden_on_the_device(cuda_device):
    import test_image_loss_host as H
    with np.load(H.GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    before = IL.stats()
    H.run_golden(g, cuda_device)
    after = IL.stats()
    assert after["fallback_calls"] == before["fallback_calls"] and after["native_calls"] > before["native_calls"]


def test_two_runs_give_equal_bits(cuda_device):
    def twice(fn):
        first = fn()
        second = fn()
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(first, second))

    for shape, name in (((1, 3, 448, 448), "soft"), ((2, 3, 33, 65), "random30"), ((1, 256, 7, 9), "none")):
        a, b, m, *_ = _l1_case(shape, name)

        def run_l1():
            la, lb = _dev(a, cuda_device, True), _dev(b, cuda_device, True)
            loss = IL.l1(la, lb, _dev(m, cuda_device))
            loss.backward()
            return loss.detach(), la.grad, lb.grad
        twice(run_l1)
    for shape in R.GAN_SHAPES:
        for real in (True, False):
            pred, label, w, *_ = _gan_case(shape, real, True)

            def run_gan():
                p = _dev(pred, cuda_device, True)
                loss = IL.gan_loss(p, _dev(label, cuda_device), _dev(w, cuda_device), real=real)
                loss.backward()
                return loss.detach(), p.grad
            twice(run_gan)


def test_operators_do_not_wait_for_the_device(cuda_device):
    """Every forward and backward under torch's sync debug mode: a synchronising call inside would raise."""
    a, b, m, *_ = _l1_case((2, 3, 33, 65), "random30")
    pred, label, w, *_ = _gan_case((2, 9, 7, 5), True, True)
    seg, mask = R.one_hot_seg(2, 8, 33, 65)
    la, lb, dm = _dev(a, cuda_device, True), _dev(b, cuda_device, True), _dev(m, cuda_device)
    p, dl, dw = _dev(pred, cuda_device, True), _dev(label, cuda_device), _dev(w, cuda_device)
    dseg, dmask = _dev(seg, cuda_device), _dev(mask, cuda_device)
    before = IL.stats()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total = IL.l1(la, lb, dm) + IL.gan_loss(p, dl, dw, real=True) + IL.gan_loss(p, dl, dw, real=False)
        total.backward()
        out = IL.label_map(dseg, (8, 16), dmask)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    after = IL.stats()
    assert after["native_calls"] == before["native_calls"] + 4 and after["fallback_calls"] == before["fallback_calls"]
    assert bool(torch.isfinite(total)) and la.grad is not None and p.grad is not None and float(out.sum()) == 2 * 8 * 16
