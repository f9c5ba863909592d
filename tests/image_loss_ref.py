"""Yardstick of the image-loss tests (CPU and GPU): core/train.py:285 (masked L1), losses/gan.py:55-97 (the N+1-label GAN
loss) and models/discriminator.py:177-189 (_smooth_interp) restated in float64 numpy, with their gradients and the terms of
the error bars, and the seeded inputs and shape lists the cases share.  Nothing here calls the code under test."""
import math

import numpy as np

U = 2.0 ** -24          # unit roundoff of float32
LOSS_REL = 1e-5         # |loss - loss64| <= LOSS_REL * T (README: the bar of this project's float32 sums)
GRAD_REL = 2.0 ** -22   # two roundings where torch's own float32 result happens to be exact

L1_SHAPES = [(1, 3, 1, 1), (1, 3, 5, 7), (2, 3, 33, 65), (1, 3, 448, 448)]
L1_WIDE_SHAPE = (1, 256, 7, 9)      # mask None only: a per-layer criterion of the perceptual loss
L1_MASKS = ("none", "ones", "zeros", "random30", "block", "soft")
GAN_SHAPES = [(1, 3, 1, 1), (2, 9, 7, 5), (3, 5, 16, 16), (1, 9, 112, 112)]      # pred: [B, C + 1, h, w]
LABEL_SIZES = [((448, 448), (112, 112)), ((29, 23), (7, 5)), ((33, 65), (8, 16)), ((4, 4), (1, 1))]
LABEL_CLASSES = (2, 8, 32)


def seed_of(*key):
    """A seed that does not depend on PYTHONHASHSEED."""
    s = 17
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


# ---- inputs ------------------------------------------------------------------------------------------------------------
def images(shape, seed=0):
    """(a, b) float32 in [-1.2, 1.2]; a twentieth of the elements equal, so that sign(0) occurs."""
    g = np.random.default_rng(seed_of("img", shape, seed))
    a = (g.random(shape) * 2.4 - 1.2).astype(np.float32)
    b = (g.random(shape) * 2.4 - 1.2).astype(np.float32)
    same = g.random(shape) < 0.05
    b[same] = a[same]
    return a, b


def make_mask(name, b, h, w, seed=0):
    """float32 [B,1,H,W] or None."""
    g = np.random.default_rng(seed_of("mask", name, b, h, w, seed))
    if name == "none":
        return None
    if name == "ones":
        return np.ones((b, 1, h, w), np.float32)
    if name == "zeros":
        return np.zeros((b, 1, h, w), np.float32)
    if name == "random30":
        return (g.random((b, 1, h, w)) < 0.3).astype(np.float32)
    if name == "block":
        m = np.ones((b, 1, h, w), np.float32)
        m[:, :, h // 4:h // 4 + max(1, h // 2), w // 3:w // 3 + max(1, w // 2)] = 0
        return m
    if name == "soft":
        return (g.random((b, 1, h, w)) * 1.5 - 0.25).astype(np.float32)   # any values: negative ones too
    raise KeyError(name)


def one_hot_seg(b, c, h, w, seed=0, hole=True):
    """(seg one-hot float32 [B,C,H,W], mask binary float32 [B,1,H,W] with a fully masked rectangle)."""
    g = np.random.default_rng(seed_of("seg", b, c, h, w, seed))
    cls = g.integers(0, c, (b, h, w))
    seg = (np.arange(c)[None, :, None, None] == cls[:, None]).astype(np.float32)
    mask = (g.random((b, 1, h, w)) < 0.8).astype(np.float32)
    if hole:
        mask[:, :, h // 4:h // 4 + max(1, h // 2), w // 4:w // 4 + max(1, w // 2)] = 0
    return seg, mask


def gan_inputs(shape, seed=0, scale=3.0, labels="onehot"):
    """(pred float32 [B,C+1,h,w], label float32 [B,C,h,w], weight float32 [B,1,h,w]).  labels: "onehot" (with pixels
    whose class is 0, which the loss ignores) or "soft" (any non-negative values)."""
    b, c1, h, w = shape
    c = c1 - 1
    g = np.random.default_rng(seed_of("gan", shape, seed))
    pred = (g.standard_normal(shape) * scale).astype(np.float32)
    if labels == "onehot":
        cls = g.integers(0, c, (b, h, w))
        label = (np.arange(c)[None, :, None, None] == cls[:, None]).astype(np.float32)
    else:
        label = g.random((b, c, h, w)).astype(np.float32)
    weight = (g.random((b, 1, h, w)) < 0.7).astype(np.float32) * (0.5 + g.random((b, 1, h, w))).astype(np.float32)
    return pred, label, weight


# ---- K20 ---------------------------------------------------------------------------------------------------------------
def l1_64(a, b, mask=None):
    """(loss, T, da, db) in float64 for float32 inputs, g = 1.  The loss sums the term in float64 (T = sum |t| / n is the
    loss itself); the gradient's sign is that of the operator's float32 term fl(fl(a m) - fl(b m)), which is what decides
    it where the two products round to one float."""
    a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
    a64, b64 = a32.astype(np.float64), b32.astype(np.float64)
    if mask is None:
        m, t32 = 1.0, a32 - b32
    else:
        m32 = np.asarray(mask, np.float32)
        m, t32 = m32.astype(np.float64), a32 * m32 - b32 * m32
    t = a64 * m - b64 * m
    n = t.size
    loss = float(np.abs(t).sum() / n)
    da = np.sign(t32).astype(np.float64) * m / n * np.ones_like(t)
    return loss, loss, da, -da


# ---- K21 ---------------------------------------------------------------------------------------------------------------
def gan64(pred, label, weight=None, real=True):
    """(loss, T, dpred) in float64, g = 1.  T = mean(weight * sum_c lab_c (|lse| + |p_c|)) in the real mode,
    mean(weight * (|lse| + |p_C|)) in the fake mode: the two operands of the difference counted apart, as they cancel."""
    p = np.array(pred, np.float64)
    lab = np.array(label, np.float64)
    b, c1, h, w = p.shape
    c = c1 - 1
    assert lab.shape == (b, c, h, w)
    p[:, 0] = 0.0
    lab[:, 0] = 0.0
    wt = np.ones((b, 1, h, w)) if weight is None else np.asarray(weight, np.float64)
    mx = p.max(axis=1, keepdims=True)
    e = np.exp(p - mx)
    ssum = e.sum(axis=1, keepdims=True)
    lse = mx + np.log(ssum)
    soft = e / ssum
    n = b * h * w
    if real:
        per = (lab * (lse - p[:, :c])).sum(axis=1, keepdims=True)
        mag = (lab * (np.abs(lse) + np.abs(p[:, :c]))).sum(axis=1, keepdims=True)
        S = lab.sum(axis=1, keepdims=True)
        target = np.concatenate([lab, np.zeros((b, 1, h, w))], axis=1)
        d = soft * S - target
    else:
        per = lse - p[:, c:]
        mag = np.abs(lse) + np.abs(p[:, c:])
        target = np.zeros_like(p)
        target[:, c] = 1.0
        d = soft - target
    d = d * wt / n
    d[:, 0] = 0.0
    return float((wt * per).sum() / n), float((np.abs(wt) * mag).sum() / n), d


def gan_grad_bound(pred, label, weight=None, real=True):
    """Per-element bound of a float32 evaluation of dpred, from the formats alone: softmax_c = exp(p_c - mx) / sum carries
    the rounding of its argument (|p_c - mx| u after exp), exp's own error (2 u allowed), C roundings of the sum and one of
    the division: (A + C + 5) u relative with A = max_c |p_c - mx| -- or, evaluated as exp(p_c - lse) the way log_softmax's
    backward does, the rounding of lse = mx + log(sum) as well, |lse| u <= (|mx| + log(C + 1)) u, so A takes both; S
    carries C u; the product, the difference, the scale g / count and the weight one rounding each, counted on
    |softmax S| + |lab|."""
    p = np.array(pred, np.float64)
    lab = np.array(label, np.float64)
    b, c1, h, w = p.shape
    p[:, 0] = 0.0
    lab[:, 0] = 0.0
    wt = np.ones((b, 1, h, w)) if weight is None else np.abs(np.asarray(weight, np.float64))
    mx = p.max(axis=1, keepdims=True)
    A = np.abs(p - mx).max(axis=1, keepdims=True) + np.abs(mx) + math.log(c1)
    e = np.exp(p - mx)
    soft = e / e.sum(axis=1, keepdims=True)
    if real:
        S = lab.sum(axis=1, keepdims=True)
        target = np.concatenate([lab, np.zeros((b, 1, h, w))], axis=1)
    else:
        S = np.ones((b, 1, h, w))
        target = np.zeros_like(p)
        target[:, c1 - 1] = 1.0
    # ... and 2^-126, float32's smallest normal number: a softmax below it is flushed or loses bits
    bound = ((A + 2 * c1 + 9) * soft * S + 4 * target) * U * wt / (b * h * w) + 2.0 ** -126
    bound[:, 0] = 0.0
    return bound


# ---- K22 ---------------------------------------------------------------------------------------------------------------
def windows(n_in, n_out):
    """adaptive_avg_pool2d's windows: [(lo, hi)] with lo = floor(i N / n), hi = ceil((i + 1) N / n)."""
    return [((i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)) for i in range(n_out)]


def label_map64(seg, size, mask=None, dtype=np.float64):
    """One-hot [B,C,h,w] float32 of the first channel with the largest window SUM of seg * mask, the sums in `dtype`."""
    x = np.asarray(seg, dtype)
    if mask is not None:
        x = x * np.asarray(mask, dtype)
    b, c, H, W = x.shape
    h, w = size
    sums = np.zeros((b, c, h, w), dtype)
    for i, (y0, y1) in enumerate(windows(H, h)):
        for j, (x0, x1) in enumerate(windows(W, w)):
            acc = np.zeros((b, c), dtype)
            for y in range(y0, y1):          # row-major, one addition at a time
                for xx in range(x0, x1):
                    acc = acc + x[:, :, y, xx]
            sums[:, :, i, j] = acc
    best = sums.argmax(axis=1)               # the first maximum
    return (np.arange(c)[None, :, None, None] == best[:, None]).astype(np.float32)


def label_map64_fast(seg, size, mask=None):
    """The same for inputs whose window sums are exact in any order (one-hot times binary): float64 prefix sums."""
    x = np.asarray(seg, np.float64)
    if mask is not None:
        x = x * np.asarray(mask, np.float64)
    b, c, H, W = x.shape
    h, w = size
    p = np.zeros((b, c, H + 1, W + 1))
    p[:, :, 1:, 1:] = x.cumsum(axis=2).cumsum(axis=3)
    ys, xs = windows(H, h), windows(W, w)
    y0, y1 = np.array([v[0] for v in ys]), np.array([v[1] for v in ys])
    x0, x1 = np.array([v[0] for v in xs]), np.array([v[1] for v in xs])
    sums = (p[:, :, y1][:, :, :, x1] - p[:, :, y0][:, :, :, x1] - p[:, :, y1][:, :, :, x0] + p[:, :, y0][:, :, :, x0])
    best = sums.argmax(axis=1)
    return (np.arange(c)[None, :, None, None] == best[:, None]).astype(np.float32)


# ---- bars ---------------------------------------------------------------------------------------------------------------
def check_loss(got, loss64, T, what):
    err = abs(float(got) - loss64)
    bar = LOSS_REL * T
    print("%s: loss %.9g ref64 %.9g |err| %.3g bar %.3g (err/bar %.3g)" % (what, float(got), loss64, err, bar, err / bar if bar else 0.0))
    assert math.isfinite(float(got)) and err <= bar, "%s: |loss - loss64| = %.3g > 1e-5 T = %.3g" % (what, err, bar)
    return err / bar if bar else 0.0


def check_grad(got, ref64, torch32, what):
    """|got - ref64| <= 4 E + 2^-22 |ref64| per element, E the largest error of torch's own float32 lines on this tensor.
    Prints got's largest error over E."""
    got, ref64, torch32 = np.asarray(got, np.float64), np.asarray(ref64), np.asarray(torch32, np.float64)
    assert got.shape == ref64.shape == torch32.shape, (what, got.shape, ref64.shape, torch32.shape)
    E = float(np.abs(torch32 - ref64).max()) if ref64.size else 0.0
    err = np.abs(got - ref64)
    bar = 4 * E + GRAD_REL * np.abs(ref64)
    worst = float(err.max()) if err.size else 0.0
    print("%s: max |err| %.3g, E (torch float32) %.3g, got/E %s" % (what, worst, E, "%.3g" % (worst / E) if E else "n/a (E = 0)"))
    assert np.all(np.isfinite(got)) and np.all(err <= bar), "%s: %d elements beyond 4 E + 2^-22 |ref|, worst excess %.3g" % (
        what, int((err > bar).sum()), float((err - bar).max()))
    return worst / E if E else 0.0
