"""-m gpu: grad_embeddings of the hash-grid encoder, element by element, on its six paths (float32 / binary16 / double,
each through the atomic kernels K10 / K10t and through the deterministic reducer K10a-c), against the float64 sum of
the kernels' own addends (tests/grid_rows.py).  The older bars of test_grid_encoder_gpu.py and test_grid_det_gpu.py
(1e-5 / 2e-2 / 1e-12 * max) stay where they are; these are the ones an element of a short list cannot hide behind.

Tier 1, every element, every path:  |got - sum64| <= ((1 + u_acc)^adds - 1) * abs64 + u_store * |sum64|, where adds is
the largest number of rounded additions any one term passes through and is read off the kernel:

  atomic (k_grid_bwd, k_grid_bwd_t)   each term is added once into an element that starts at zero.  0 + t is exact and
      every later add rounds once in the element's format, so adds = n - 1 whatever order the hardware picks.
      u_acc = 2^-24 / 2^-11 / 2^-53; a binary16 sum in the subnormal range is exact (both operands are multiples of
      2^-24), so the relative form needs no floor.  An element with n = 1 must therefore be the term, bit for bit.
  deterministic (k_det_reduce)   one level of the reducer, for the term of one lane:
      * the segmented scan over the wave, `for (d = 1; d < 64; d <<= 1)`: 6 steps, each at most one det_combine_left
        (x = left + x) on the partial sum that holds the term                                              -> 6
      * across the four waves, `for (k = 0; k < 3; k++)`: R = agg[k], or R + agg[k] when wave k continues the run.  A
        term of wave 0 passes through the adds for k = 1 and k = 2 before wave 3 reads R                   -> 2
      * `det_combine_left(R, x)`: R joins the lane's own partial sum                                        -> 1
      9 per level, as gce_det.h's header counts them; a record carries the partial sum to the next level, where it is
      an entry like any other, for det_levels(L * B * 2^D) levels (det_layout's recurrence).  Every one of these adds
      joins two non-empty partial sums of the same row (det_combine_left skips an absent side), so a row of n terms
      has n - 1 of them in all, and no term passes through more than min(n - 1, 9 * levels).  That is tighter than
      9 * levels + 1 for the short rows (an n = 1 row is exact here too), and it is what det_adds uses.  The closing
      `old + sum` is exact into a zeroed table; into a table that held values it is one more rounding, u * |old + sum|
      on top (old is then one more addend of sum64 and abs64).  u_acc = 2^-24 for float32 AND binary16 tables (DetAcc:
      binary16 terms are summed in float), 2^-53 for double; the binary16 store rounds once more, u_store = 2^-11 (in
      the binary16 subnormal range it is exact: float sums of multiples of 2^-24 are multiples of 2^-24).
  The reference's own accumulation error (grid_rows.ref_bound: float64 sums of 24-bit terms, longdouble sums of the
  double path's) is added to the bound; it is 2^-29 / 2^-11 of it.

Tier 2, float32, both paths: median, 99th percentile and maximum of |got - sum64| / (2^-24 * abs64) over the elements
with n >= 2, each within 4 x what the C oracle (a sequential float32 sum in id order) leaves on the same case.  Tier 1
is blunt on lists of thousands; this tier is what bites there.  An entry of LIMITS above 4 is twice a measured ratio
and names its cause; tools/grid_rows.py writes the measured ratios to profiles/grid_rows.jsonl.
"""
import numpy as np
import pytest
import torch

import grid_rows as GR
from gaussiancity_amd import grid_encoder as GE

pytestmark = pytest.mark.gpu

DTYPES = {"float": np.float32, "half": np.float16, "double": np.float64}
# (case, path, statistic) -> limit where the chosen summation form needs more than GR.M = 4 (see the module docstring)
LIMITS = {}

RUNS = ([(c, p, "float") for c in GR.F32_CASES for p in GR.PATHS]
        + [(c, p, "double") for c in GR.F64_CASES for p in GR.PATHS]
        + [(c, "atomic", "half") for c in GR.F16_CASES] + [(c, "det", "half") for c in GR.F16_DET_CASES])


def _tier1(c, path, T, got, nonzero_start=False, label=""):
    """Asserts tier 1 and its consequences on a result; returns (sum64, abs64, n)."""
    sum64, abs64, n, bound = GR.path_bound(c, path, T, nonzero_start)
    assert got.shape == sum64.shape and got.dtype == T
    worst, bad = GR.tier1(got, sum64, abs64, n, bound)
    print("%s %s %s%s: n==0 %d rows, n==1 %d rows, longest list %d; tier 1: worst %.3f of the bound, %d elements beyond" % (
        c.name, path, np.dtype(T).name, label, int((n == 0).sum()), int((n == 1).sum()), int(n.max()), worst, bad))
    if not nonzero_start:
        assert not got[n == 0].any(), "a row that no point touches is not an exact zero"
        if path == "atomic":
            one = n == 1
            assert np.array_equal(got[one], sum64[one].astype(T)), "a row with one contribution is not that term, bit for bit"
    assert bad == 0, "%d elements beyond the summation bound (worst %.3g x)" % (bad, worst)
    return sum64, abs64, n


@pytest.mark.parametrize("name,path,dt", RUNS, ids=["%s-%s-%s" % r for r in RUNS])
def test_every_element_of_the_table_gradient(cuda_device, name, path, dt):
    c, T = GR.case(name), DTYPES[dt]
    got = GR.gpu_backward(c, path, T, cuda_device)
    sum64, abs64, n = _tier1(c, path, T, got)
    if T != np.float32:
        return
    _, ost = c.oracle()
    st = GR.stats(GR.units(got, sum64, abs64, GR.U[T]), n)
    r = GR.ratios(st, ost)
    print("%s %s tier 2 over %d elements: gpu %s, oracle %s, ratios median %.2f p99 %.2f max %.2f" % (
        name, path, st["elements"], {k: round(st[k], 3) for k in GR.STATS}, {k: round(ost[k], 3) for k in GR.STATS},
        r["median"], r["p99"], r["max"]))
    assert st["elements"] == ost["elements"]
    assert GR.within(st, ost, {k: LIMITS[(name, path, k)] for k in GR.STATS if (name, path, k) in LIMITS}), r


@pytest.mark.parametrize("name,dt", [("A-d3", "float"), ("A-d3", "half"), ("A-d3", "double"), ("C-c8", "float")])
def test_deterministic_pass_into_a_table_that_holds_values(cuda_device, name, dt):
    """A starting table of normal values with every third row -0.0: a touched element is old + sum within the bound plus
    one rounding, an untouched one keeps its bits (the sign of -0.0 included)."""
    c, T = GR.case(name), DTYPES[dt]
    old = c.table0.astype(T)
    got = GR.gpu_backward(c, "det", T, cuda_device, table0=c.table0)
    _, _, n = _tier1(c, "det", T, got, nonzero_start=True, label=" (non-zero start)")
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[np.dtype(T).itemsize]
    assert (n == 0).sum() > 20 and np.signbit(old[n == 0]).any()
    assert np.array_equal(got[n == 0].view(bits), old[n == 0].view(bits)), "an untouched row was rewritten"


@pytest.mark.parametrize("path", GR.PATHS)
def test_module_backward_at_the_production_level_shape(cuda_device, path):
    """Case B through GridEncoder(...).backward: the autograd node's [B, L*C] -> [L, B, C] layout of grad and its scaling
    (none) are under tier 1 too.  The module maps [-1, 1] to [0, 1] as (x + 1) / 2 in float32; the case's points are
    that expression's results, formed here the same way."""
    c = GR.case("B")
    enc = GE.GridEncoder(c.D, c.L, c.C, 128, base_resolution=16, log2_hashmap_size=19).to(cuda_device)
    assert tuple(enc.embeddings.shape) == (c.rows, c.C) and np.array_equal(enc.offsets.cpu().numpy(), c.offsets)
    assert np.log2(enc.per_level_scale) == c.S and enc.base_resolution == c.H
    xin = (c.x * np.float32(2) - np.float32(1)).astype(np.float32)
    unit = ((xin + np.float32(1)) / np.float32(2)).astype(np.float32)
    m = GR.Case("B")
    m.x = unit
    g = np.ascontiguousarray(m.grad(np.float32).transpose(1, 0, 2).reshape(c.B, c.L * c.C))
    try:
        GE.set_deterministic(path == "det")
        GE.reset_stats()
        enc(torch.from_numpy(xin).to(cuda_device)).backward(torch.from_numpy(g).to(cuda_device))
        assert GE.stats() == {"atomic_backward_calls": int(path == "atomic"), "deterministic_backward_calls": int(path == "det")}
    finally:
        GE.set_deterministic(None)
    _tier1(m, path, np.float32, enc.embeddings.grad.cpu().numpy(), label=" (module)")
