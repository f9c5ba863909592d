"""-m gpu: the spconv SubMConv3d and torch_scatter segment_csr drop-ins (spconv/, torch_scatter/ ->
gaussiancity_amd.sparse -> include/gcs.h -> gfx950 kernels) against the float64 reference tests/sparse_ref.py.
Bar: |got - ref| <= 1e-5 * scale element by element (scale = sum of |terms|); bit-exact where the rule is a copy
(one unit tap, min / max of segment_csr); bit-identical between two runs (no float atomics)."""
import copy

import numpy as np
import pytest
import torch

import sparse_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_s
    _native_s.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def shell():
    return R.pool_stages(R.shell_cloud(16384, 2024), 4)


def _close(got, ref, scale, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = err > TOL * scale
    assert not bad.any(), "%s: %d elements off, worst %g at scale %g" % (
        what, int(bad.sum()), float(err[bad].max()), float(scale[bad][np.argmax(err[bad])]))


def _run(dev, idx, shape, batch, x, w, b, k, dil, dy, key=None):
    """Forward + backward through the drop-in; returns y, dx, dw, db as numpy."""
    import spconv.pytorch as spconv
    conv = spconv.SubMConv3d(x.shape[1], w.shape[0], k, dilation=dil, bias=b is not None, indice_key=key).to(dev)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w))
        if b is not None:
            conv.bias.copy_(torch.from_numpy(b))
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    t = spconv.SparseConvTensor(xt, torch.from_numpy(idx).to(dev), shape, batch)
    out = conv(t)
    out.features.backward(torch.from_numpy(dy).to(dev))
    g = lambda p: None if p is None else p.grad.cpu().numpy()  # noqa: E731
    return out.features.detach().cpu().numpy(), xt.grad.cpu().numpy(), g(conv.weight), g(conv.bias)


def _check_case(dev, idx, shape, batch, cin, cout, k, dil=1, bias=True, seed=0, what=""):
    rng = np.random.default_rng(seed)
    n = len(idx)
    x = rng.normal(size=(n, cin)).astype(np.float32)
    w = (rng.normal(size=(cout, k, k, k, cin)) / np.sqrt(cin * k ** 3)).astype(np.float32)
    b = rng.normal(size=cout).astype(np.float32) if bias else None
    dy = rng.normal(size=(n, cout)).astype(np.float32)
    y, dx, dw, db = _run(dev, idx, shape, batch, x, w, b, k, dil, dy)
    nbr = R.neighbours(idx, shape, (k,) * 3, (dil,) * 3)
    ry, sy = R.conv_forward(x, w, b, nbr)
    (rdx, sdx), (rdw, sdw), (rdb, sdb) = R.conv_backward(x, w, nbr, dy)
    assert y.shape == (n, cout) and dx.shape == (n, cin) and dw.shape == w.shape
    _close(y, ry, sy, what + " forward")
    _close(dx, rdx, sdx, what + " dX")
    _close(dw, rdw, sdw, what + " dW")
    if bias:
        _close(db, rdb, sdb, what + " dB")
    return nbr


@pytest.mark.parametrize("k,dil", [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_orientation_one_unit_tap_is_an_exact_shift(dev, k, dil):
    import spconv.pytorch as spconv
    ext = 12
    rng = np.random.default_rng(k + 10 * dil)
    coords = np.unique(rng.integers(0, ext, (900, 3)), axis=0)
    idx = R.with_batch(coords, rng.integers(0, 2, len(coords)))
    idx = idx[np.unique(R.pack(idx, (ext,) * 3), return_index=True)[1]]
    C_ = 6
    x = rng.normal(size=(len(idx), C_)).astype(np.float32)
    nbr = R.neighbours(idx, (ext,) * 3, (k,) * 3, (dil,) * 3)
    K = k ** 3
    for tap in (0, 1, K // 2 - 1, K // 2 + k, K - 1):
        conv = spconv.SubMConv3d(C_, C_, k, dilation=dil, bias=False).to(dev)
        w = np.zeros((C_, K, C_), np.float32)
        w[np.arange(C_), tap, np.arange(C_)] = 1.0
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(w.reshape(C_, k, k, k, C_)))
        t = spconv.SparseConvTensor(torch.from_numpy(x).to(dev), torch.from_numpy(idx).to(dev), [ext] * 3, 2)
        got = conv(t).features.detach().cpu().numpy()
        want = np.where(nbr[:, tap:tap + 1] >= 0, x[np.maximum(nbr[:, tap], 0)], 0.0).astype(np.float32)
        assert (nbr[:, tap] >= 0).sum() > 20
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, dil, tap)


@pytest.mark.parametrize("cin,cout,k,stage", R.PTV3_SHAPES)
def test_ptv3_shapes_forward_and_backward(dev, shell, cin, cout, k, stage):
    coords = shell[stage]
    idx = R.with_batch(coords, np.zeros(len(coords)))
    shape = (coords.max(0) + 3).tolist()
    nbr = _check_case(dev, idx, shape, 1, cin, cout, k, bias=(k == 3), seed=cin + k, what="%d->%d k%d" % (cin, cout, k))
    assert (nbr >= 0).sum(1).mean() > 3   # surface-like neighbourhoods


@pytest.mark.parametrize("cin,cout", [(3, 5), (1, 1)])
def test_odd_channel_counts(dev, cin, cout):
    rng = np.random.default_rng(cin)
    coords = R.shell_cloud(700, cin, extent=40)
    idx = R.with_batch(coords, rng.integers(0, 2, len(coords)))
    _check_case(dev, idx, [40, 40, 40], 2, cin, cout, 3, seed=cin, what="%d->%d" % (cin, cout))


@pytest.mark.parametrize("n", [0, 1, 17])
@pytest.mark.parametrize("k", [3, 5])
def test_tiny_clouds_two_batches_near_the_bounds(dev, n, k):
    rng = np.random.default_rng(n + k)
    shape = [5, 6, 7]
    coords = np.stack([rng.choice([0, 1, s - 2, s - 1], n) for s in shape], 1) if n else np.zeros((0, 3), np.int64)
    idx = R.with_batch(coords, rng.integers(0, 2, n))
    idx = idx[np.sort(np.unique(R.pack(idx, shape), return_index=True)[1])] if n else idx.astype(np.int32)
    _check_case(dev, idx, shape, 2, 4, 3, k, dil=1, seed=n, what="n=%d" % n)


def test_duplicate_voxels(dev):
    rng = np.random.default_rng(7)
    coords = R.shell_cloud(3000, 7, extent=60)
    extra = coords[rng.integers(0, len(coords), 330)]
    coords = np.concatenate([coords, extra])[rng.permutation(3330)]
    idx = R.with_batch(coords, np.zeros(len(coords)))
    keys = R.pack(idx, (60, 60, 60))
    assert len(np.unique(keys)) < len(keys) - 250
    for cin, cout in ((16, 24), (64, 64)):
        nbr = _check_case(dev, idx, [60, 60, 60], 1, cin, cout, 3, seed=cin, what="duplicates %d" % cin)
        rng2 = np.random.default_rng(cin)
        x = rng2.normal(size=(len(idx), cin)).astype(np.float32)
        w = rng2.normal(size=(cout, 3, 3, 3, cin)).astype(np.float32)
        y = _run(dev, idx, [60, 60, 60], 1, x, w, None, 3, 1, np.zeros((len(idx), cout), np.float32))[0]
        order = np.argsort(keys, kind="stable")
        same = keys[order][1:] == keys[order][:-1]
        a, b = order[1:][same], order[:-1][same]
        assert np.array_equal(y[a].view(np.uint32), y[b].view(np.uint32)), "rows of one voxel differ"
        assert np.array_equal(nbr[a], nbr[b])


def test_rulebook_reuse_and_build_counter(dev):
    import spconv.pytorch as spconv
    from gaussiancity_amd import sparse as SP
    coords = R.shell_cloud(2000, 3, extent=50)
    idx = torch.from_numpy(R.with_batch(coords, np.zeros(len(coords)))).to(dev)
    t = spconv.SparseConvTensor(torch.randn(len(coords), 8, device=dev), idx, [50, 50, 50], 1)
    a = spconv.SubMConv3d(8, 8, 3, indice_key="s0").to(dev)
    b = spconv.SubMConv3d(8, 8, 3, indice_key="s0").to(dev)
    SP.reset_stats()
    u = b(a(t))
    assert SP.stats()["rulebook_builds"] == 1 and "s0" in t.indice_dict and u.indice_dict is t.indice_dict
    v = a(t.replace_feature(torch.randn(len(coords), 8, device=dev)))
    assert SP.stats()["rulebook_builds"] == 1 and v.features.shape == (len(coords), 8)
    with pytest.raises(ValueError):
        spconv.SubMConv3d(8, 8, 5, indice_key="s0").to(dev)(u)
    with pytest.raises(ValueError):
        spconv.SubMConv3d(8, 8, 3, dilation=2, indice_key="s0").to(dev)(u)
    spconv.SubMConv3d(8, 8, 3).to(dev)(u)
    spconv.SubMConv3d(8, 8, 3).to(dev)(u)
    assert SP.stats()["rulebook_builds"] == 3      # indice_key=None builds every call


def test_index_errors_are_clean(dev):
    import spconv.pytorch as spconv
    conv = spconv.SubMConv3d(2, 2, 3).to(dev)
    f = torch.zeros(3, 2, device=dev)
    for bad, shape, batch in (([[0, 1, 1, 1], [0, 9, 1, 1], [0, 2, 2, 2]], [8, 8, 8], 1),
                              ([[0, 1, 1, 1], [1, 1, 1, 1], [0, -1, 2, 2]], [8, 8, 8], 2),
                              ([[0, 1, 1, 1], [2, 1, 1, 1], [0, 2, 2, 2]], [8, 8, 8], 2)):
        t = spconv.SparseConvTensor(f, torch.tensor(bad, dtype=torch.int32, device=dev), shape, batch)
        with pytest.raises(ValueError):
            conv(t)
    t = spconv.SparseConvTensor(f, torch.zeros(3, 4, dtype=torch.int32, device=dev), [2 ** 30] * 3, 64)
    with pytest.raises(ValueError):
        conv(t)
    # a non-contiguous features view is accepted
    idx = torch.tensor([[0, 1, 1, 1], [0, 1, 1, 2], [0, 2, 2, 2]], dtype=torch.int32, device=dev)
    g = torch.randn(2, 3, device=dev).t()
    assert tuple(conv(spconv.SparseConvTensor(g, idx, [8, 8, 8], 1)).features.shape) == (3, 2)


def test_determinism_512_channels(dev, shell):
    coords = shell[0]
    idx = R.with_batch(coords, np.zeros(len(coords)))
    rng = np.random.default_rng(5)
    x = rng.normal(size=(len(idx), 512)).astype(np.float32)
    w = (rng.normal(size=(512, 3, 3, 3, 512)) / 100).astype(np.float32)
    b = rng.normal(size=512).astype(np.float32)
    dy = rng.normal(size=(len(idx), 512)).astype(np.float32)
    first = _run(dev, idx, [160] * 3, 1, x, w, b, 3, 1, dy)
    second = _run(dev, idx, [160] * 3, 1, x, w, b, 3, 1, dy)
    for p, q, name in zip(first, second, ("y", "dx", "dw", "db")):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), name


@pytest.mark.parametrize("reduce", ["sum", "add", "mean", "min", "max"])
@pytest.mark.parametrize("trail", [(), (5,), (3, 4)])
def test_segment_csr(dev, reduce, trail):
    import torch_scatter
    rng = np.random.default_rng(len(trail))
    counts = rng.integers(0, 6, 300)
    counts[[0, 7, 299]] = 0                      # empty segments, first and last among them
    indptr = np.concatenate([[0], np.cumsum(counts)])
    m = int(indptr[-1]) + 4                      # rows after the last segment get no gradient
    src = rng.integers(-3, 4, (m,) + trail).astype(np.float32)   # small integers: many ties
    if reduce in ("sum", "add", "mean"):
        src += rng.normal(size=src.shape).astype(np.float32)
    s = torch.from_numpy(src).to(dev).requires_grad_(True)
    out = torch_scatter.segment_csr(s, torch.from_numpy(indptr).to(dev), reduce=reduce)
    dout = rng.normal(size=out.shape).astype(np.float32)
    out.backward(torch.from_numpy(dout).to(dev))
    ref, sc, arg = R.segment_csr(src, indptr, reduce)
    dref = R.segment_csr_backward(dout, indptr, reduce, arg, src.shape)
    got, dgot = out.detach().cpu().numpy(), s.grad.cpu().numpy()
    assert got.shape == ref.shape and dgot.shape == src.shape
    if reduce in ("min", "max"):
        assert np.array_equal(got, ref.astype(np.float32)) and np.array_equal(dgot, dref.astype(np.float32))
    else:
        _close(got, ref, sc, reduce)
        dsc = R.segment_csr_backward(np.abs(dout), indptr, reduce, arg, src.shape)
        _close(dgot, dref, dsc, reduce + " gradient")


# ---- a PTv3-shaped stack, evaluated on the GPU through the drop-ins and in float64 on the CPU -----------------
class _Stack(torch.nn.Module):
    def __init__(self):
        super().__init__()
        import spconv.pytorch as spconv
        self.stem = spconv.SubMConv3d(128, 32, 5, bias=False, indice_key="stem")
        self.lin0 = torch.nn.Linear(32, 32)
        self.ln0 = torch.nn.LayerNorm(32)
        self.c0a = spconv.SubMConv3d(32, 32, 3, indice_key="stage0")
        self.c0b = spconv.SubMConv3d(32, 32, 3, indice_key="stage0")
        self.pool = torch.nn.Linear(32, 64)
        self.c1a = spconv.SubMConv3d(64, 64, 3, indice_key="stage1")
        self.c1b = spconv.SubMConv3d(64, 64, 3, indice_key="stage1")
        self.up = torch.nn.Linear(64, 32)
        self.c0c = spconv.SubMConv3d(32, 32, 3, indice_key="stage0")


def _cpu_conv(mod, t):
    idx = t.indices.numpy()
    nbr = torch.from_numpy(R.neighbours(idx, t.spatial_shape, mod.kernel_size, mod.dilation))
    W = mod.weight.reshape(mod.out_channels, -1, mod.in_channels)
    y = t.features.new_zeros((len(idx), mod.out_channels))
    if mod.bias is not None:
        y = y + mod.bias
    for k in range(W.shape[1]):
        rows = (nbr[:, k] >= 0).nonzero()[:, 0]
        y = y.index_add(0, rows, t.features[nbr[rows, k]] @ W[:, k, :].t())
    return t.replace_feature(y)


def _cpu_segment(src, indptr, reduce):
    counts = indptr[1:] - indptr[:-1]
    seg = torch.repeat_interleave(torch.arange(len(counts)), counts)
    if reduce == "mean":
        return src.new_zeros((len(counts),) + src.shape[1:]).index_add(0, seg, src) / counts.clamp(min=1)[:, None]
    return src.new_zeros((len(counts),) + src.shape[1:]).scatter_reduce(0, seg[:, None].expand_as(src), src, "amax",
                                                                        include_self=False)


def _stack_loss(m, feats, idx, shape, gpu, probe):
    import spconv.pytorch as spconv
    import torch_scatter
    conv = (lambda mod, t: mod(t)) if gpu else _cpu_conv
    seg = torch_scatter.segment_csr if gpu else _cpu_segment
    t = spconv.SparseConvTensor(feats, idx, shape, 1)
    t = conv(m.stem, t)
    t = t.replace_feature(m.ln0(m.lin0(t.features)))
    t = conv(m.c0b, conv(m.c0a, t))
    f = m.pool(t.features)
    code, inverse = torch.unique(idx.long() >> 1, dim=0, return_inverse=True)
    order = torch.argsort(inverse, stable=True)
    counts = torch.bincount(inverse, minlength=len(code))
    indptr = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
    pooled = seg(f[order], indptr, reduce="max")
    centre = seg(idx[order].to(f.dtype)[:, 1:], indptr, reduce="mean")
    p = spconv.SparseConvTensor(pooled, code.int(), [(s >> 1) + 1 for s in shape], 1)
    p = conv(m.c1b, conv(m.c1a, p))
    t = t.replace_feature(m.up(p.features[inverse]))
    t = conv(m.c0c, t)
    return (t.features * probe).sum() + 1e-3 * (centre ** 2).sum(), centre


def test_ptv3_shaped_stack_against_float64(dev):
    from gaussiancity_amd import sparse as SP
    coords = R.shell_cloud(3000, 11, extent=64)
    idx = R.with_batch(coords, np.zeros(len(coords)))
    rng = np.random.default_rng(11)
    feats = rng.normal(size=(len(idx), 128)).astype(np.float32)
    probe = rng.normal(size=(len(idx), 32)).astype(np.float32)
    torch.manual_seed(0)
    m = _Stack()
    m64 = copy.deepcopy(m).double()
    m = m.to(dev)
    SP.reset_stats()
    loss, centre = _stack_loss(m, torch.from_numpy(feats).to(dev), torch.from_numpy(idx).to(dev), [64] * 3, True,
                               torch.from_numpy(probe).to(dev))
    loss.backward()
    assert SP.stats()["rulebook_builds"] == 3
    loss64, centre64 = _stack_loss(m64, torch.from_numpy(feats).double(), torch.from_numpy(idx), [64] * 3, False,
                                   torch.from_numpy(probe).double())
    loss64.backward()
    assert abs(loss.item() - loss64.item()) <= 1e-4 * abs(loss64.item())
    assert torch.allclose(centre.cpu().double(), centre64, rtol=1e-6, atol=1e-5)
    for (name, p), (_, q) in zip(m.named_parameters(), m64.named_parameters()):
        g, h = p.grad.cpu().double(), q.grad
        assert float((g - h).abs().max()) <= 1e-4 * float(h.abs().max()), name
