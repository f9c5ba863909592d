"""The image losses without a GPU (include/gcv.h K20-K22, gaussiancity_amd/image_loss.py): the CPU path against the float64
restatement of tests/image_loss_ref.py and against upstream's recorded results (tests/golden/image_loss.npz), GANLoss's
assertions and list form, install / uninstall on a stub module, the counters, and the library's entry points with every
argument error."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import image_loss_ref as R
from gaussiancity_amd import _native_v as V
from gaussiancity_amd import image_loss as IL

INVALID = -1  # GCV_ERR_INVALID_ARGUMENT
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_loss.npz")
FORMS = {"dis_real": (True, True), "dis_fake": (False, True), "gen_real": (True, False)}


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _t(a, grad=False):
    return None if a is None else torch.from_numpy(np.array(a)).requires_grad_(grad)


# ---- the CPU path against the float64 restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.L1_SHAPES[:3] + [R.L1_WIDE_SHAPE], ids=str)
def test_l1_cpu_against_float64(shape):
    a, b = R.images(shape)
    before = IL.stats()
    masks = ("none",) if shape == R.L1_WIDE_SHAPE else R.L1_MASKS
    for name in masks:
        m = R.make_mask(name, shape[0], shape[2], shape[3])
        loss64, T, da64, db64 = R.l1_64(a, b, m)
        ta, tb = _t(a, True), _t(b, True)
        loss = IL.l1(ta, tb, _t(m))
        assert loss.dim() == 0 and loss.dtype == torch.float32
        R.check_loss(loss.item(), loss64, T, "cpu l1 %s %s" % (shape, name))
        loss.backward()
        for got, want in ((ta.grad, da64), (tb.grad, db64)):     # sign * m / count: one division, one product
            assert np.all(np.abs(got.numpy() - want) <= R.GRAD_REL * np.abs(want))
        if name == "zeros":
            assert loss.item() == 0.0 and not ta.grad.any() and not tb.grad.any()
    after = IL.stats()
    assert after["fallback_calls"] == before["fallback_calls"] + len(masks) and after["native_calls"] == before["native_calls"]


@pytest.mark.parametrize("shape", R.GAN_SHAPES[:3], ids=str)
@pytest.mark.parametrize("real", [True, False])
def test_gan_loss_cpu_against_float64(shape, real):
    for labels, scale in (("onehot", 3.0), ("soft", 3.0), ("onehot", 50.0)):
        pred, label, weight = R.gan_inputs(shape, scale=scale, labels=labels)
        for w in (None, weight):
            what = "cpu gan %s real=%s %s x%g %s" % (shape, real, labels, scale, "w" if w is not None else "nw")
            loss64, T, d64 = R.gan64(pred, label, w, real)
            p = _t(pred, True)
            loss = IL.gan_loss(p, _t(label), _t(w), real=real)
            assert loss.dim() == 0
            R.check_loss(loss.item(), loss64, T, what)
            loss.backward()
            err = np.abs(p.grad.numpy() - d64)
            bound = R.gan_grad_bound(pred, label, w, real)
            print("%s: gradient worst err/bound %.3g" % (what, float((err / np.maximum(bound, 1e-300)).max())))
            assert np.all(err <= bound)
            assert not p.grad[:, 0].any(), what + ": channel 0 of dpred is not exactly zero"


@pytest.mark.parametrize("src,dst", R.LABEL_SIZES[1:], ids=str)
@pytest.mark.parametrize("c", R.LABEL_CLASSES)
def test_label_map_cpu_bit_for_bit(src, dst, c):
    seg, mask = R.one_hot_seg(2, c, *src)
    for m in (None, mask):
        want = R.label_map64(seg, dst, m)
        assert np.array_equal(want, R.label_map64(seg, dst, m, dtype=np.float32))     # exact sums: any precision agrees
        assert np.array_equal(want, R.label_map64_fast(seg, dst, m))
        got = IL.label_map(_t(seg), dst, _t(m))
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, c) + tuple(dst)
        assert np.array_equal(got.numpy(), want)
        assert np.array_equal(got.numpy().sum(axis=1), np.ones((2,) + tuple(dst), np.float32))
    # a window that is masked out entirely gives channel 0
    got = IL.label_map(_t(seg), dst, _t(np.zeros_like(mask))).numpy()
    assert got[:, 0].all() and not got[:, 1:].any()


def test_label_map_tie_goes_to_the_lower_channel():
    seg = np.zeros((1, 4, 4, 4), np.float32)
    seg[0, 3, :2], seg[0, 1, 2:] = 1.0, 1.0          # channels 3 and 1 cover half of the one window each
    got = IL.label_map(_t(seg), (1, 1)).numpy().reshape(-1)
    assert got.tolist() == [0.0, 1.0, 0.0, 0.0]
    assert np.array_equal(R.label_map64(seg, (1, 1)).reshape(-1), got)


def test_label_map_refuses_a_gradient():
    seg = torch.zeros(1, 2, 4, 4, requires_grad=True)
    with pytest.raises(RuntimeError):
        IL.label_map(seg, (2, 2))
    with torch.no_grad():
        assert not IL.label_map(seg, (2, 2)).requires_grad
    assert tuple(IL.label_map(seg.detach(), (8, 8)).shape) == (1, 2, 8, 8)      # larger than the source: torch's lines


# ---- against upstream's recorded results ---------------------------------------------------------------------------------
def check_golden_loss(got, loss32, loss64, what):
    """Within 4x the reference's own float32 error of its float64 run."""
    loss32, loss64 = (float(np.asarray(v).reshape(-1)[0]) for v in (loss32, loss64))     # the list form records [1]
    err, bar = abs(float(got) - loss64), 4 * abs(loss32 - loss64)
    print("%s: loss %.9g ref64 %.9g |err| %.3g, 4 x reference float32 error %.3g" % (what, float(got), float(loss64), err, bar))
    assert err <= bar, "%s: |loss - ref64| = %.3g > 4 x |ref32 - ref64| = %.3g" % (what, err, bar)


def golden_gan_cases(g):
    for key in sorted({k.rsplit("/", 1)[0] for k in g if k.startswith("gan/") and k.count("/") == 4}):
        _, shape, form, wname = key.split("/")
        base = "gan/" + shape
        yield key, form, g[base + "/pred"], g[base + "/label"], (g[base + "/weight"] if wname == "w" else None)


def run_golden(g, device):
    """Every recorded case through the public functions on `device`."""
    crit = IL.GANLoss()
    n = 0
    for key, form, pred, label, weight in golden_gan_cases(g):
        t_real, dis_update = FORMS[form]
        p = _t(pred).to(device).requires_grad_(True)
        w = None if weight is None else _t(weight).to(device)
        loss = crit({"pred": p, "label": _t(label).to(device)}, t_real, w, dis_update=dis_update)
        loss.backward()
        check_golden_loss(loss.item(), g[key + "/loss32"], g[key + "/loss64"], key)
        R.check_grad(p.grad.cpu().numpy(), g[key + "/dpred64"], g[key + "/dpred32"], key + " dpred")
        n += 1
    assert n == 12
    ps = [_t(g["gan_list/pred%d" % i]).to(device).requires_grad_(True) for i in range(2)]
    xs = [{"pred": p, "label": _t(g["gan_list/label%d" % i]).to(device)} for i, p in enumerate(ps)]
    loss = crit([[xs[1], xs[0]], xs[1]], True, _t(g["gan_list/weight"]).to(device), dis_update=True)
    assert tuple(loss.shape) == (1,)
    loss.sum().backward()
    check_golden_loss(loss.item(), g["gan_list/loss32"], g["gan_list/loss64"], "gan_list")
    for i, p in enumerate(ps):
        R.check_grad(p.grad.cpu().numpy(), g["gan_list/dpred%d_64" % i], g["gan_list/dpred%d_32" % i], "gan_list dpred%d" % i)
    for key in sorted({k.rsplit("/", 1)[0] for k in g if k.startswith("interp/")}):
        h, w = (int(v) for v in key.split("_")[1].split("x"))
        seg, mask = _t(g[key + "/seg"].astype(np.float32)).to(device), _t(g[key + "/mask"].astype(np.float32)).to(device)
        assert np.array_equal(g[key + "/out32"], g[key + "/out64"])
        for got in (IL.label_map(seg, (h, w), mask), IL.label_map(seg * mask, (h, w))):
            assert np.array_equal(got.cpu().numpy().astype(np.uint8), g[key + "/out64"]), key
    fake, rgb = _t(g["l1/fake"]).to(device).requires_grad_(True), _t(g["l1/rgb"]).to(device).requires_grad_(True)
    loss = IL.l1(fake, rgb, _t(g["l1/msk"]).to(device))
    loss.backward()
    check_golden_loss(loss.item(), g["l1/loss32"], g["l1/loss64"], "l1")
    R.check_grad(fake.grad.cpu().numpy(), g["l1/dfake64"], g["l1/dfake32"], "l1 dfake")
    R.check_grad(rgb.grad.cpu().numpy(), g["l1/drgb64"], g["l1/drgb32"], "l1 drgb")


def test_golden_on_the_cpu(golden):
    before = IL.stats()["native_calls"]
    run_golden(golden, torch.device("cpu"))
    assert IL.stats()["native_calls"] == before


def test_restatement_against_the_golden(golden):
    """The float64 restatement is upstream's float64 run to float64 rounding."""
    for key, form, pred, label, weight in golden_gan_cases(golden):
        loss64, T, d64 = R.gan64(pred, label, weight, FORMS[form][0])
        assert abs(loss64 - float(golden[key + "/loss64"])) <= 1e-13 * T
        assert np.all(np.abs(d64 - golden[key + "/dpred64"]) <= 1e-13 * np.abs(d64).max())
    loss64, T, da, db = R.l1_64(golden["l1/fake"], golden["l1/rgb"], golden["l1/msk"])
    assert abs(loss64 - float(golden["l1/loss64"])) <= 1e-13 * T
    assert np.array_equal(da, golden["l1/dfake64"]) and np.array_equal(db, golden["l1/drgb64"])
    for key in sorted({k.rsplit("/", 1)[0] for k in golden if k.startswith("interp/")}):
        h, w = (int(v) for v in key.split("_")[1].split("x"))
        want = R.label_map64(golden[key + "/seg"].astype(np.float32), (h, w), golden[key + "/mask"].astype(np.float32))
        assert np.array_equal(want.astype(np.uint8), golden[key + "/out64"])


# ---- GANLoss ---------------------------------------------------------------------------------------------------------------
def test_gan_loss_module_assertions_and_forms():
    pred, label, weight = (_t(v) for v in R.gan_inputs((2, 9, 7, 5)))
    crit = IL.GANLoss()
    assert crit.real_label == 1.0 and crit.fake_label == 0.0 and IL.GANLoss(0.9, 0.1).real_label == 0.9
    x = {"pred": pred, "label": label}
    with pytest.raises(AssertionError):
        crit(x, True, reduce_dim=False)
    with pytest.raises(AssertionError, match="GAN loss must be aiming for real."):
        crit(x, False, dis_update=False)
    with pytest.raises(AssertionError):
        crit({"pred": pred[:, :8], "label": label}, True)
    assert torch.equal(crit(x, True, weight), IL.gan_loss(pred, label, weight, real=True))
    assert torch.equal(crit(x, True, weight, dis_update=False), IL.gan_loss(pred, label, weight, real=True))
    assert torch.equal(crit(x, False, weight), IL.gan_loss(pred, label, weight, real=False))
    assert torch.equal(crit.loss(x, True, weight, True, True), crit(x, True, weight))
    other = {"pred": pred * 0.5, "label": label}
    got = crit([[x, other], x], True, weight)
    want = (IL.gan_loss(other["pred"], label, weight) + IL.gan_loss(pred, label, weight)) / 2
    assert tuple(got.shape) == (1,) and torch.equal(got[0], want)
    assert torch.equal(IL.gan_loss(pred, label, 0.5), IL.gan_loss(pred, label) * 0.5)       # a number as the weight: torch's lines


# ---- install / uninstall --------------------------------------------------------------------------------------------------
def _stub_modules():
    gan, dis = types.ModuleType("stub_losses_gan"), types.ModuleType("stub_models_discriminator")

    class GANLoss(torch.nn.Module):
        def forward(self, input_x, t_real, weight=None, reduce_dim=True, dis_update=True):
            return self.loss(input_x, t_real, weight, reduce_dim, dis_update)

        def loss(self, input_x, t_real, weight=None, reduce_dim=True, dis_update=True):
            return "stub loss"

    class Discriminator(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.interpolator = self._smooth_interp

        @staticmethod
        def _smooth_interp(x, size):
            return "stub interp"

    gan.GANLoss, dis.Discriminator = GANLoss, Discriminator
    return gan, dis


def test_install_and_uninstall_on_a_stub_module():
    gan, dis = _stub_modules()
    pred, label, weight = (_t(v) for v in R.gan_inputs((2, 9, 7, 5)))
    seg, mask = (_t(v) for v in R.one_hot_seg(1, 8, 29, 23))
    x = {"pred": pred, "label": label}
    early = dis.Discriminator()
    original_loss, original_interp = gan.GANLoss.loss, dis.Discriminator.__dict__["_smooth_interp"]
    IL.install(gan, dis)
    IL.install(gan, dis)                                    # idempotent: the originals are not lost
    assert getattr(gan, IL._ORIGINAL_LOSS) is original_loss and getattr(dis, IL._ORIGINAL_INTERP) is original_interp
    assert torch.equal(gan.GANLoss()(x, False, weight), IL.gan_loss(pred, label, weight, real=False))
    with pytest.raises(AssertionError, match="aiming for real"):
        gan.GANLoss()(x, False, dis_update=False)
    late = dis.Discriminator()
    assert torch.equal(late.interpolator(seg * mask, size=(7, 5)), IL.label_map(seg, (7, 5), mask))
    assert torch.equal(dis.Discriminator._smooth_interp(seg, (7, 5)), IL.label_map(seg, (7, 5)))
    assert early.interpolator(seg, size=(7, 5)) == "stub interp"       # built before install: keeps the module's own
    IL.uninstall(gan, dis)
    IL.uninstall(gan, dis)
    assert gan.GANLoss.loss is original_loss and dis.Discriminator.__dict__["_smooth_interp"] is original_interp
    assert not hasattr(gan, IL._ORIGINAL_LOSS) and not hasattr(dis, IL._ORIGINAL_INTERP)
    assert gan.GANLoss()(x, True) == "stub loss" and dis.Discriminator().interpolator(seg, (7, 5)) == "stub interp"
    IL.install(gan_module=gan)                              # one module at a time
    assert gan.GANLoss.loss is not original_loss and dis.Discriminator.__dict__["_smooth_interp"] is original_interp
    IL.uninstall(gan)
    assert gan.GANLoss.loss is original_loss


def test_stats_and_fallback_reasons():
    IL.reset_stats()
    assert IL.stats() == {"native_calls": 0, "fallback_calls": 0}
    a, b = (_t(v) for v in R.images((1, 3, 5, 7)))
    IL.l1(a, b)
    IL.l1(a.double(), b.double())
    pred, label, weight = (_t(v) for v in R.gan_inputs((1, 3, 1, 1)))
    IL.gan_loss(pred, label, weight)
    IL.label_map(label, (1, 1))
    assert IL.stats() == {"native_calls": 0, "fallback_calls": 4}
    s = IL.stats()
    s["fallback_calls"] = 99                                # a copy
    assert IL.stats()["fallback_calls"] == 4
    IL.reset_stats()
    assert IL.stats() == {"native_calls": 0, "fallback_calls": 0}
    assert IL.max_classes() == 32


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
NAMES = ("gcv_image_loss_max_classes", "gcv_image_loss_partials", "gcv_mean_abs_forward", "gcv_mean_abs_backward", "gcv_gan_loss_forward",
         "gcv_gan_loss_backward", "gcv_label_map")


def test_library_exports_the_entry_points():
    lib = V.lib()
    assert set(NAMES) <= set(V.EXPORTED_SYMBOLS)
    assert lib.gcv_image_loss_max_classes() == 32
    assert lib.gcv_image_loss_partials(1, 0) == 1 and lib.gcv_image_loss_partials(4096, 0) == 1 and lib.gcv_image_loss_partials(4097, 0) == 2
    assert lib.gcv_image_loss_partials(3 * 448 * 448, 0) == 147 and lib.gcv_image_loss_partials(112 * 112, 1) == 49
    assert lib.gcv_image_loss_partials(0, 0) == 0 and b"gcv_image_loss_partials" in lib.gcv_last_error()
    assert lib.gcv_image_loss_partials(2 ** 31, 1) == 0


S3, S2 = C.c_int64 * 3, C.c_int64 * 2
A, B_, M, P, L, O, O2 = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000   # never dereferenced


def _l1_forward(lib, **o):
    """gcv_mean_abs_forward for a contiguous 1 x 3 x 8 x 8 pair with a mask, some arguments replaced."""
    a = dict(a=A, sa=S3(192, 64, 8), b=B_, sb=S3(192, 64, 8), m=M, sm=S2(64, 8), B=1, C=3, H=8, W=8, part=P, n=1, loss=L)
    a.update(o)
    return lib.gcv_mean_abs_forward(a["a"], a["sa"], a["b"], a["sb"], a["m"], a["sm"], a["B"], a["C"], a["H"], a["W"], a["part"], a["n"],
                              a["loss"], None)


def _l1_backward(lib, **o):
    a = dict(a=A, sa=S3(192, 64, 8), b=B_, sb=S3(192, 64, 8), m=M, sm=S2(64, 8), B=1, C=3, H=8, W=8, g=L, da=O, db=O2)
    a.update(o)
    return lib.gcv_mean_abs_backward(a["a"], a["sa"], a["b"], a["sb"], a["m"], a["sm"], a["B"], a["C"], a["H"], a["W"], a["g"], a["da"],
                               a["db"], None)


def _gan(lib, backward, **o):
    """pred 1 x 9 x 8 x 8, label 1 x 8 x 8 x 8, weight 1 x 1 x 8 x 8, contiguous."""
    a = dict(p=A, sp=S3(576, 64, 8), l=B_, sl=S3(512, 64, 8), w=M, sw=S2(64, 8), B=1, C=8, H=8, W=8, real=1, part=P, n=1, loss=L,
             g=L, d=O)
    a.update(o)
    head = (a["p"], a["sp"], a["l"], a["sl"], a["w"], a["sw"], a["B"], a["C"], a["H"], a["W"], a["real"])
    if backward:
        return lib.gcv_gan_loss_backward(*head, a["g"], a["d"], None)
    return lib.gcv_gan_loss_forward(*head, a["part"], a["n"], a["loss"], None)


def _label(lib, **o):
    a = dict(s=A, ss=S3(512, 64, 8), m=M, sm=S2(64, 8), B=1, C=8, H=8, W=8, h=2, w=2, out=O)
    a.update(o)
    return lib.gcv_label_map(a["s"], a["ss"], a["m"], a["sm"], a["B"], a["C"], a["H"], a["W"], a["h"], a["w"], a["out"], None)


ERRORS = [
    (_l1_forward, dict(a=None), b"null"), (_l1_forward, dict(b=None), b"null"), (_l1_forward, dict(sa=None), b"null"),
    (_l1_forward, dict(sm=None), b"null"), (_l1_forward, dict(part=None), b"null"), (_l1_forward, dict(loss=None), b"null"),
    (_l1_forward, dict(H=0), b"positive"), (_l1_forward, dict(C=-1), b"positive"),
    (_l1_forward, dict(B=2 ** 15, C=2 ** 10, H=8, W=8), b"2^31"),
    (_l1_forward, dict(sa=S3(192, -64, 8)), b"negative stride"), (_l1_forward, dict(a=A + 2), b"misaligned"),
    (_l1_forward, dict(part=P + 4), b"misaligned"),
    (_l1_forward, dict(loss=A + 4 * 191), b"overlap"), (_l1_forward, dict(part=M), b"overlap"), (_l1_forward, dict(part=L), b"overlap"),
    (_l1_forward, dict(H=64, W=64, sa=S3(12288, 4096, 64), sb=S3(12288, 4096, 64), sm=S2(4096, 64), n=2), b"gcv_image_loss_partials"),
    (_l1_backward, dict(g=None), b"null"), (_l1_backward, dict(da=None, db=None), b"null"), (_l1_backward, dict(a=None), b"null"),
    (_l1_backward, dict(da=A), b"overlap"), (_l1_backward, dict(db=O + 4), b"overlap"), (_l1_backward, dict(da=M - 4), b"overlap"),
    (_l1_backward, dict(W=0), b"positive"),
    (lambda lib, **o: _gan(lib, False, **o), dict(p=None), b"null"), (lambda lib, **o: _gan(lib, False, **o), dict(l=None), b"null"),
    (lambda lib, **o: _gan(lib, False, **o), dict(loss=None), b"null"), (lambda lib, **o: _gan(lib, False, **o), dict(C=33), b"max_classes"),
    (lambda lib, **o: _gan(lib, False, **o), dict(C=0), b"positive"), (lambda lib, **o: _gan(lib, False, **o), dict(part=A + 4 * 574), b"overlap"),
    (lambda lib, **o: _gan(lib, False, **o), dict(n=0), b"gcv_image_loss_partials"),
    (lambda lib, **o: _gan(lib, True, **o), dict(d=None), b"null"), (lambda lib, **o: _gan(lib, True, **o), dict(g=None), b"null"),
    (lambda lib, **o: _gan(lib, True, **o), dict(C=33), b"max_classes"), (lambda lib, **o: _gan(lib, True, **o), dict(d=B_ + 4 * 511), b"overlap"),
    (lambda lib, **o: _gan(lib, True, **o), dict(sl=S3(512, 64, -8)), b"negative stride"),
    (_label, dict(s=None), b"null"), (_label, dict(out=None), b"null"), (_label, dict(ss=None), b"null"), (_label, dict(C=33), b"max_classes"),
    (_label, dict(h=9), b"exceeds"), (_label, dict(w=0), b"positive"), (_label, dict(out=A + 4 * 511), b"overlap"),
    (_label, dict(out=M), b"overlap"),
]


@pytest.mark.parametrize("call,over,word", ERRORS, ids=lambda v: None if callable(v) else ("-".join(sorted(v)) if isinstance(v, dict) else v.decode()))
def test_argument_errors_come_back_before_anything_is_queued(call, over, word):
    """No GPU is present here: a call that got as far as a launch would report a HIP error (-2), not -1 or -4."""
    lib = V.lib()
    rc = call(lib, **over)
    msg = lib.gcv_last_error()
    assert rc == (-4 if word == b"gcv_image_loss_partials" else INVALID), (rc, msg)
    assert msg.startswith(b"gcv_") and word in msg, msg
