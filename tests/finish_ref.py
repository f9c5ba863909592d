"""Yardstick of the frame-finish tests (CPU and GPU): the road-mask blur of scripts/inference.py:255,264-272 restated in
float64 numpy with explicit reflect indexing, the video byte of :665 in float64, the error bounds, and the seeded
images and masks the cases share.  Nothing here calls the code under test."""
import functools

import numpy as np

ROAD = 1            # synth.LAYOUT_CLASSES["ROAD"]
U = 2.0 ** -24      # unit roundoff of float32


def gamma(n):
    """gamma_n = n u / (1 - n u): the bound of n accumulated float32 roundings."""
    return n * U / (1.0 - n * U)


def reflect(i, n):
    """torch's "reflect" padding index, the edge not repeated: -1 -> 1, n -> n - 2."""
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def road_mask(ins_map, b, road_id=ROAD, flip=False):
    """bool [B,H,W] from an [H,W] or [B,H,W] map."""
    m = np.asarray(ins_map)
    m = np.broadcast_to(m if m.ndim == 3 else m[None], (b,) + m.shape[-2:])
    if flip:
        m = m[..., ::-1]
    return m == road_id


def blur64(img, weights):
    """(sum of w x, sum of |w x|) in float64 over the reflected (2r+1)^2 neighbourhood of every pixel of [...,H,W]."""
    x = np.asarray(img, np.float64)
    w = np.asarray(weights, np.float64)          # the float32 weights, cast
    k = w.shape[0]
    r, (h, wd) = k // 2, x.shape[-2:]
    s, sa = np.zeros_like(x), np.zeros_like(x)
    for dy in range(k):
        iy = reflect(np.arange(h) + dy - r, h)
        for dx in range(k):
            ix = reflect(np.arange(wd) + dx - r, wd)
            t = w[dy, dx] * x[..., iy[:, None], ix[None, :]]
            s += t
            sa += np.abs(t)
    return s, sa


def finish64(img, ins_map, weights, road_id=ROAD, flip=False):
    """(out float64 [B,3,H,W], road bool [B,H,W], bound float64 [B,3,H,W]) for a float32 image [3,H,W] / [B,3,H,W]: road
    pixels the float64 sum, others the input; bound = gamma_(k*k) * sum |w x|, the road-pixel error bound of a float32
    evaluation with one rounding per product and per addition (any order)."""
    x = np.asarray(img)
    x4 = x if x.ndim == 4 else x[None]
    road = road_mask(ins_map, x4.shape[0], road_id, flip)
    s, sa = blur64(x4, weights)
    out = np.where(road[:, None], s, x4.astype(np.float64))
    return out, road, gamma(np.asarray(weights).size) * sa


def byte64(v):
    """The real number (clamp(v, -1, 1) / 2 + 0.5) * 255 in float64; the video byte is its integer part."""
    return (np.clip(np.asarray(v, np.float64), -1.0, 1.0) / 2.0 + 0.5) * 255.0


def check_float(got, img, out64, road, bound, what=""):
    """got float32 [B,3,H,W] (numpy): non-road pixels bit for bit the input, road pixels within the bound.  Prints the
    largest road error relative to its bound before asserting."""
    got, img = np.asarray(got), np.asarray(img)
    img4 = img if img.ndim == 4 else img[None]
    got4 = got if got.ndim == 4 else got[None]
    assert got4.shape == img4.shape and got4.dtype == np.float32, (what, got4.shape, got4.dtype)
    r3 = np.broadcast_to(road[:, None], got4.shape)
    assert np.array_equal(got4.view(np.int32)[~r3], np.ascontiguousarray(img4).view(np.int32)[~r3]), what + ": a non-road pixel changed"
    err = np.abs(got4.astype(np.float64) - out64)[r3]
    if err.size:
        ratio = float((err / np.maximum(bound[r3], 1e-300)).max())
        print("%s: road pixels %d, max |err| %.3g, max err/bound %.3f" % (what, err.size // 3, float(err.max()), ratio))
        assert np.all(err <= bound[r3]), (what, ratio)


def check_bytes(got_u8, out64, bound, bgr=False, what="", max_fraction=0.01):
    """got uint8 [B,H,W,3]: every byte within 1 of the float64 frame's byte, a difference of 1 only where the float64 value
    lies within 255 * (bound / 2 + 3 * 2^-24) of an integer; fewer than 1 % of the bytes may use that allowance."""
    g = np.asarray(got_u8)
    g = g if g.ndim == 4 else g[None]
    t = byte64(out64).transpose(0, 2, 3, 1)
    allow = (255.0 * (bound / 2.0 + 3.0 * U)).transpose(0, 2, 3, 1)
    if bgr:
        t, allow = t[..., ::-1], allow[..., ::-1]
    assert g.shape == t.shape and g.dtype == np.uint8, (what, g.shape, g.dtype)
    diff = np.abs(g.astype(np.int64) - np.floor(t).astype(np.int64))
    near = np.abs(t - np.rint(t)) <= allow
    used = diff == 1
    print("%s: bytes %d, off by one %d, largest difference %d" % (what, g.size, int(used.sum()), int(diff.max())))
    assert diff.max() <= 1, (what, int(diff.max()))
    assert np.all(near[used]), what + ": a byte is off by one away from an integer boundary"
    assert used.mean() < max_fraction, (what, float(used.mean()))
    return int(used.sum())


MASKS = ("all", "none", "checker", "corners_edges", "random30")


def make_mask(name, h, w, seed=0):
    """int16 [H,W]: ROAD where the named pattern says so, other ids (0, 2..9, one large) elsewhere."""
    rng = np.random.default_rng(1000 + seed)
    m = rng.integers(2, 10, size=(h, w)).astype(np.int16)
    m[rng.random((h, w)) < 0.1] = 0
    m[rng.random((h, w)) < 0.05] = 257           # low byte 1: only a 16-bit comparison tells it from ROAD
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "all":
        road = np.ones((h, w), bool)
    elif name == "none":
        road = np.zeros((h, w), bool)
    elif name == "checker":
        road = (yy + xx) % 2 == 0
    elif name == "corners_edges":
        road = np.zeros((h, w), bool)
        for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)):
            road[y, x] = True
    elif name == "random30":
        road = rng.random((h, w)) < 0.3
    else:
        raise KeyError(name)
    m[road] = ROAD
    return m


@functools.lru_cache(maxsize=None)
def image(h, w, b=0, seed=0):
    """float32 [3,H,W] (b = 0) or [b,3,H,W], uniform in [-1.5, 1.5] so that the clamp of the byte path is exercised."""
    rng = np.random.default_rng(77 + seed + 131 * h + w)
    a = rng.uniform(-1.5, 1.5, size=((b,) if b else ()) + (3, h, w)).astype(np.float32)
    a.setflags(write=False)
    return a


# (H, W, kernel_size): the smallest shapes at which the indexing can go wrong
SHAPES = ((2, 2, 3), (3, 5, 3), (37, 70, 3), (64, 64, 3), (65, 129, 3), (4, 4, 7), (6, 9, 5))
