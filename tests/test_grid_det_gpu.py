"""-m gpu: the deterministic table gradient of the hash-grid encoder (gce_backward_det, include/gce.h ABI v3; kernels in
gaussiancity_amd/csrc/gce_det.h).  Bars: grad_embeddings max|d| <= 1e-5 * max(1, max|ref|) in float32 (the project's bar
for this output; a strictly sequential float32 sum in id order stays at 0.05 - 0.20 of it on these shapes), 1e-12 * max in
double, 2e-2 * max in half; grad_inputs bit-exact as with the atomic path; and every result BIT-IDENTICAL from run to run,
across streams and whatever the workspace held.  The per-element bar of the same output -- every element within the
summation bound of its own terms -- is tests/test_grid_rows_gpu.py; the bars here stay as they are."""
import ctypes
import math

import numpy as np
import pytest
import torch

import grid_util as GU
from gaussiancity_amd import _native_e as E
from gaussiancity_amd import grid_encoder as GE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def go():
    from oracle import grid_oracle as GO
    GO.lib()
    return GO


def _bar(got, ref, rel=1e-5):
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    scale = max(1.0, float(np.abs(ref.astype(np.float64)).max()))
    print("max|d| = %.3e  bar = %.3e" % (err, rel * scale))
    return err <= rel * scale


class _Case:
    """One problem on the device; backward() runs one table-gradient pass and returns (grad_embeddings, grad_inputs)."""

    def __init__(self, dev, x, rows, offsets, S, H, grad, gridtype, align, dtype=torch.float32):
        self.dev, self.B, self.D = dev, x.shape[0], x.shape[1]
        self.L, self.C, self.rows = len(offsets) - 1, grad.shape[2], rows
        self.S, self.H, self.gridtype, self.align, self.dtype = S, H, gridtype, align, dtype
        self.x, self.off, self.grad = (torch.from_numpy(a).to(dev) for a in (x, offsets, grad))
        self.table = torch.zeros(rows, self.C, device=dev, dtype=dtype)   # `embeddings`: only its dtype is used

    def backward(self, calc=False, dd=None, table0=None, workspace=None, det=True):
        ge = torch.zeros_like(self.table) if table0 is None else table0.clone()
        gi = torch.zeros((self.B, self.D) if calc else (1,), device=self.dev, dtype=self.dtype)
        dd = dd if calc else torch.empty(1, device=self.dev, dtype=self.dtype)
        args = (self.grad, self.x, self.table, self.off, ge, self.B, self.D, self.C, self.L, self.S, self.H, calc, dd, gi,
                self.gridtype, self.align)
        if det:
            GE.ext_backward_deterministic(*args, workspace=workspace)
        else:
            GE.ext_backward(*args)
        return ge, gi

    def workspace_bytes(self):
        return int(E.lib().gce_backward_det_workspace_bytes(self.B, self.D, self.L, self.rows))


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


@pytest.mark.parametrize("D,C,gridtype,align,lh", [(2, 1, 0, False, 9), (3, 4, 1, True, 13), (4, 2, 0, True, 10), (5, 8, 0, False, 9)])
def test_parity_float32(cuda_device, go, D, C, gridtype, align, lh):
    rng = np.random.default_rng(100 * D + C)
    L, B = 5, 3001
    x, emb, offsets, S, H = GU.make_case(rng, B, D, C, L, base=3, desired=50, log2_hashmap=lh, align_corners=align)
    grad = rng.normal(size=(L, B, C)).astype(np.float32)
    _, dd_o = go.forward(x, emb, offsets, S, H, True, gridtype, align)
    ge_o, gi_o = go.backward(grad, x, emb.shape, offsets, S, H, dd_o, gridtype, align)
    case = _Case(cuda_device, x, emb.shape[0], offsets, S, H, grad, gridtype, align)
    dd = torch.from_numpy(dd_o.reshape(B, -1)).to(cuda_device)
    ge, gi = case.backward(calc=True, dd=dd)
    assert _bar(ge.cpu().numpy(), ge_o)
    assert np.array_equal(gi.cpu().numpy().view(np.uint32), gi_o.view(np.uint32)), "grad_inputs not bit-exact"
    ge2, _ = case.backward(calc=False)
    assert _same_bits(ge2, ge), "the table gradient depends on calc_grad_inputs"


@pytest.mark.parametrize("C,gridtype", [(8, 1), (1, 0)])
def test_long_lists_and_run_to_run_bits(cuda_device, C, gridtype):
    """16 / 32 / 88 rows per level under 20 000 points: lists of thousands of contributions (18 001 on the longest row), so
    runs cross many tiles and the record levels are used.  Reference: float64 autograd."""
    rng = np.random.default_rng(31 + C)
    B, D, L = 20000, 2, 3
    x, emb, offsets, S, H = GU.make_case(rng, B, D, C, L, base=2, desired=8, log2_hashmap=10)
    assert [int(offsets[i + 1] - offsets[i]) for i in range(L)] == [16, 32, 88]
    grad = rng.normal(size=(L, B, C)).astype(np.float32)
    scales = (ctypes.c_float * L)()
    assert E.lib().gce_level_scales(L, S, H, scales) == 0
    et = torch.from_numpy(emb).double().requires_grad_(True)
    out = GU.torch_reference(torch.from_numpy(x).double(), et, offsets, list(scales), gridtype, False)
    out.backward(torch.from_numpy(grad).double().permute(1, 0, 2).reshape(B, L * C))
    ref = et.grad.numpy()
    case = _Case(cuda_device, x, emb.shape[0], offsets, S, H, grad, gridtype, False)
    ge, _ = case.backward()
    assert _bar(ge.cpu().numpy(), ref)
    for _ in range(2):
        assert _same_bits(case.backward()[0], ge), "two runs differ"
    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        ge_s, _ = case.backward()
    side.synchronize()
    assert _same_bits(ge_s, ge), "a run on another stream differs"
    ws = torch.full((case.workspace_bytes(),), 0xFF, dtype=torch.uint8, device=cuda_device)
    assert _same_bits(case.backward(workspace=ws)[0], ge), "the result depends on what the workspace held"


def test_accumulates_once_into_the_table(cuda_device):
    rng = np.random.default_rng(5)
    B, D, C, L = 3001, 3, 4, 5
    x, emb, offsets, S, H = GU.make_case(rng, B, D, C, L, base=3, desired=50, log2_hashmap=13)
    grad = rng.normal(size=(L, B, C)).astype(np.float32)
    case = _Case(cuda_device, x, emb.shape[0], offsets, S, H, grad, 0, False)
    s, _ = case.backward()
    # rows that some point touches: those the atomic path turns into NaN when every gradient is NaN
    nan_case = _Case(cuda_device, x, emb.shape[0], offsets, S, H, np.full_like(grad, np.nan), 0, False)
    touched = torch.isnan(nan_case.backward(det=False)[0]).any(dim=1)
    assert 0 < int(touched.sum()) < emb.shape[0] - 100
    assert bool(torch.isnan(nan_case.backward()[0][touched]).all()) and not bool(s[~touched].any())
    g0 = torch.from_numpy(rng.normal(size=emb.shape).astype(np.float32)).to(cuda_device)
    g0[::3] = -0.0   # -0.0 + 0.0 is +0.0: a row that is rewritten as old + 0 instead of being left alone loses the sign
    got, _ = case.backward(table0=g0)
    assert _same_bits(got[touched], (g0 + s)[touched]), "not old + sum with one rounding"
    assert _same_bits(got[~touched], g0[~touched]), "an untouched row was written"
    plain = g0.abs() > 0   # and away from the -0.0 entries the whole table is g0 + S, bit for bit
    assert _same_bits(got[plain], (g0 + s)[plain])


@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_edges_small_batches(cuda_device, go, B):
    rng = np.random.default_rng(B)
    D, C, L = 3, 2, 2
    x, emb, offsets, S, H = GU.make_case(rng, B, D, C, L, base=3, desired=9, log2_hashmap=9)   # x[0] = 0.0, x[1] = 1.0
    grad = rng.normal(size=(L, B, C)).astype(np.float32)
    ge_o, _ = go.backward(grad, x, emb.shape, offsets, S, H, None, 0, False)
    case = _Case(cuda_device, x, emb.shape[0], offsets, S, H, grad, 0, False)
    ge, _ = case.backward()
    assert _bar(ge.cpu().numpy(), ge_o)
    assert _same_bits(case.backward()[0], ge)


def test_edges_every_point_out_of_range(cuda_device):
    rng = np.random.default_rng(9)
    B, D, C, L = 300, 3, 2, 2
    x, emb, offsets, S, H = GU.make_case(rng, B, D, C, L, base=3, desired=9, log2_hashmap=9)
    x[:, 1] = np.where(np.arange(B) % 2 == 0, np.float32(-0.25), np.float32(1.0000001))
    grad = rng.normal(size=(L, B, C)).astype(np.float32)
    case = _Case(cuda_device, x, emb.shape[0], offsets, S, H, grad, 0, False)
    g0 = torch.from_numpy(rng.normal(size=emb.shape).astype(np.float32)).to(cuda_device)
    g0[::2] = -0.0
    got, _ = case.backward(table0=g0)
    assert _same_bits(got, g0), "out-of-range points changed the table"


@pytest.mark.parametrize("dtype", [np.float16, np.float64], ids=["half", "double"])
@pytest.mark.parametrize("D,C,gridtype,align,lh", [(3, 2, 0, False, 9), (5, 8, 0, False, 11)])
def test_half_and_double_tables(cuda_device, dtype, D, C, gridtype, align, lh):
    from oracle import grid_oracle_typed as GT
    rng = np.random.default_rng(7 * D + C)
    L, B = 4, 1777
    x, emb32, offsets, S, H = GU.make_case(rng, B, D, C, L, base=3, desired=40, log2_hashmap=lh, align_corners=align)
    emb = emb32.astype(dtype)
    grad = rng.normal(size=(L, B, C)).astype(dtype)
    _, dd_o = GT.forward(x, emb, offsets, S, H, True, gridtype, align)
    ge_o, gi_o = GT.backward(grad, x, emb.shape, offsets, S, H, dd_o, gridtype, align)
    tdt = torch.float16 if dtype == np.float16 else torch.float64
    case = _Case(cuda_device, x, emb.shape[0], offsets, S, H, grad, gridtype, align, dtype=tdt)
    dd = torch.from_numpy(dd_o.reshape(B, -1)).to(cuda_device)
    ge, gi = case.backward(calc=True, dd=dd)
    bits = np.uint16 if dtype == np.float16 else np.uint64
    assert np.array_equal(gi.cpu().numpy().view(bits), gi_o.view(bits)), "grad_inputs not bit-exact"
    assert _bar(ge.cpu().numpy(), ge_o, 1e-12 if dtype == np.float64 else 2e-2)
    assert _same_bits(case.backward(calc=True, dd=dd)[0], ge), "two runs differ"


def test_module_at_gaussiancity_configuration(cuda_device, go, monkeypatch):
    """models/generator.py:37-42 / config.py:34: D = 5, 16 levels x 8 channels, 2^19 rows per level, 16 384 points."""
    enc = GE.GridEncoder(5, 16, 8, 2048).to(cuda_device)
    torch.manual_seed(11)
    x = torch.rand(16384, 5, device=cuda_device) * 2 - 1
    g = torch.randn(16384, 128, device=cuda_device)
    before = torch.are_deterministic_algorithms_enabled()

    def step():
        enc.embeddings.grad = None
        enc(x).backward(g)
        return enc.embeddings.grad

    try:
        GE.set_deterministic(True)
        GE.reset_stats()
        g1 = step().clone()
        g2 = step()
        assert GE.stats() == {"atomic_backward_calls": 0, "deterministic_backward_calls": 2}
        assert _same_bits(g1, g2), "two training steps gave different table gradients"
        S, H = math.log2(enc.per_level_scale), enc.base_resolution
        grad_lbc = np.ascontiguousarray(g.reshape(16384, 16, 8).permute(1, 0, 2).cpu().numpy())
        ge_o, _ = go.backward(grad_lbc, ((x + 1) / 2).cpu().numpy(), tuple(enc.embeddings.shape), enc.offsets.cpu().numpy(), S, H)
        assert _bar(g1.cpu().numpy(), ge_o)
        GE.set_deterministic(None)
        monkeypatch.setattr(GE, "_ENV_DETERMINISTIC", None)   # no GCE_DETERMINISTIC: torch's switch decides
        torch.use_deterministic_algorithms(True)
        GE.reset_stats()
        assert _same_bits(step(), g1)
        assert GE.stats() == {"atomic_backward_calls": 0, "deterministic_backward_calls": 1}
        torch.use_deterministic_algorithms(False)
        GE.set_deterministic(False)
        GE.reset_stats()
        g3 = step()
        assert GE.stats() == {"atomic_backward_calls": 1, "deterministic_backward_calls": 0}
        assert _bar(g3.cpu().numpy(), ge_o)
    finally:
        GE.set_deterministic(None)
        torch.use_deterministic_algorithms(before)
