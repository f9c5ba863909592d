"""Not gpu: the per-element reference, statistic and bounds of the hash-grid table gradient (tests/grid_rows.py) -- that
the reference forms the terms the kernels form, that the C oracle (a correct float32 evaluation) meets the bounds the GPU
tests apply, and that four subtly wrong kernels, each inside the older 1e-5 * max bar, do not."""
import numpy as np
import pytest

import grid_rows as GR
import grid_util as GU
from oracle import grid_oracle_typed as GT

U32 = GR.U[np.float32]


def _brute(grad, x, rows, offsets, S, H, gridtype, align, T):
    """One contribution at a time, in Python: point by point through _locate / _grid_index, scalar float32 weights."""
    L, B, C = grad.shape
    D = x.shape[1]
    sc = GT.level_scales(L, S, H)
    tot, tot_abs, n = np.zeros((rows, C), np.longdouble), np.zeros((rows, C), np.longdouble), np.zeros(rows, np.int64)
    for l in range(L):
        hs, res = int(offsets[l + 1] - offsets[l]), int(np.ceil(sc[l])) + 1
        for b in range(B):
            inside, pos, pg = GT._locate(x[b:b + 1], sc[l], align)
            if not inside[0]:
                continue
            for corner in range(1 << D):
                w, pl = np.float32(1.0), pg.copy()
                for d in range(D):
                    if corner >> d & 1:
                        w = np.float32(w * pos[0, d])
                        pl[0, d] += np.uint32(1)
                    else:
                        w = np.float32(w * np.float32(np.float32(1.0) - pos[0, d]))
                row = int(GT._grid_index(gridtype, align, hs, res, pl, 1)[0]) + int(offsets[l])
                n[row] += 1
                for ch in range(C):
                    g = grad[l, b, ch]
                    if T == np.float32:
                        t = np.float32(w * g)
                    elif T == np.float16:
                        t = np.float16(np.float32(w * np.float32(g)))
                    else:
                        t = np.float64(w) * g
                    tot[row, ch] += np.longdouble(t)
                    tot_abs[row, ch] += abs(np.longdouble(t))
    return tot, tot_abs, n


@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.float64], ids=["float", "half", "double"])
@pytest.mark.parametrize("D,gridtype,align", [(2, 0, False), (2, 1, True), (5, 0, True), (5, 1, False)])
def test_reference_equals_a_loop_over_the_contributions(D, gridtype, align, dtype):
    rng = np.random.default_rng(17 * D + gridtype)
    B, C, L = 23, 2, 3
    x, emb, offsets, S, H = GU.make_case(rng, B, D, C, L, base=2, desired=9, log2_hashmap=6, align_corners=align,
                                         oob_fraction=0.2)
    x[5, 0] = np.float32(2.0 ** -30)   # a weight far below the others
    grad = rng.normal(size=(L, B, C)).astype(dtype)
    rows = int(offsets[-1])
    sum64, abs64, n = GR.terms_reference(grad, x, rows, offsets, S, H, gridtype, align, dtype)
    bs, ba, bn = _brute(grad, x, rows, offsets, S, H, gridtype, align, dtype)
    assert np.array_equal(n, bn) and 0 < n.sum() < L * B * (1 << D)   # some points are out of range
    tol = 2.0 ** -50 * ba   # two float64 (longdouble in double) sums of the same terms in two orders
    assert np.all(np.abs(sum64 - bs) <= tol) and np.all(np.abs(abs64 - ba) <= tol)
    assert sum64.shape == (rows, C) and n.shape == (rows,)


@pytest.mark.parametrize("name", ["A-d2", "A-d3", "E-d3"])
def test_float32_reference_against_the_typed_oracle_in_double(name):
    """grid_oracle_typed.backward with a double gradient multiplies (double)w * g and sums in float64: only the rounding
    of the term to float32 differs, half an ulp of each."""
    c = GR.case(name)
    sum64, abs64, n = c.reference(np.float32)
    ge, _ = GT.backward(c.grad(np.float32).astype(np.float64), c.x, (c.rows, c.C), c.offsets, c.S, c.H, None, c.gridtype,
                        c.align)
    assert ge.dtype == np.float64
    assert np.all(np.abs(ge - sum64) <= U32 * abs64 + GR.ref_bound(n, abs64))
    assert np.all(ge[n == 0] == 0) and float(np.abs(ge - sum64).max()) > 0


@pytest.mark.parametrize("name", GR.F32_CASES)
def test_c_oracle_meets_the_bounds_of_every_gpu_case(name):
    """The C oracle sums each element's terms one after the other in float32: n - 1 roundings, the atomic path's count."""
    c = GR.case(name)
    sum64, abs64, n = c.reference(np.float32)
    ge, st = c.oracle()
    bound = GR.hard_bound(n, abs64, sum64, U32, GR.atomic_adds(n)) + GR.ref_bound(n, abs64)
    worst, bad = GR.tier1(ge, sum64, abs64, n, bound)
    print("%s: rows %d, n==0 %d, n==1 %d, longest %d; tier 1 worst %.3f; units %s" % (
        name, c.rows, int((n == 0).sum()), int((n == 1).sum()), int(n.max()), worst, st))
    assert bad == 0 and worst <= 1.0
    one = n == 1
    assert np.array_equal(ge[one], sum64[one].astype(np.float32)), "a single term is not returned as it is"
    assert not ge[n == 0].any()
    assert GR.within(st, st) and st["max"] <= max(1, int(n.max()) - 1)   # tier 1, first order, in units


def test_cases_reach_what_they_are_for():
    n = {k: GR.case(k).reference(np.float32)[2] for k in GR.F32_CASES}
    for k in ("A-d2", "A-d3", "A-d4", "A-d5"):
        share = (n[k] == 1).sum() / max(1, (n[k] > 0).sum())
        assert 0.005 <= share <= 0.25 and n[k].max() > 100, (k, share, n[k].max())
    assert GR.case("B").rows == 2097152 and 2 <= n["B"].max() <= 8
    assert [int(o) for o in np.diff(GR.case("C-c8").offsets)] == [16, 32, 88] and n["C-c1"].max() > 15000
    assert GR.det_levels(GR.case("C-c8").contributions) == 3 and GR.det_levels(16 * 16384 * 32) == 4
    assert GR.det_levels(256) == 1 and GR.det_levels(257) == 2
    # weights down to the float32 subnormals (D = 5; three factors of 2^-30 end at 1e-26); binary16 terms subnormal and
    # alone on their row
    for k, floor in (("E-d5", np.finfo(np.float32).tiny), ("E-d3", np.float32(1e-25))):
        c = GR.case(k)
        w = np.concatenate([w for _, _, _, w in GR._contributions(c.x, c.offsets, c.S, c.H, c.gridtype, c.align)])
        assert 0 < w[w > 0].min() < floor, (k, w[w > 0].min())
        _, abs16, n16 = c.reference(np.float16)
        assert ((abs16 > 0) & (abs16 < np.finfo(np.float16).tiny) & (n16 == 1)[:, None]).sum() > 20, k


# --------------------------------------------------------------------------------------------------- mutants
def _keep_bits(a, bits):
    m, e = np.frexp(a)
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)


MUTANTS = {
    "terms kept to 16 mantissa bits": dict(term_fn=lambda t: _keep_bits(t, 16)),
    "terms below 1e-6 flushed to zero": dict(term_fn=lambda t: np.where(np.abs(t) < 1e-6, 0.0, t)),
    "corners with a weight below 1e-6 dropped": dict(weight_fn=lambda w: (w, w >= 1e-6)),
    "weights kept to 20 mantissa bits": dict(weight_fn=lambda w: (_keep_bits(w, 20).astype(np.float32), np.ones(len(w), bool))),
}


def _verdict(c, got):
    """The GPU tests' two tiers on a float32 result of the atomic path -> list of what fails."""
    sum64, abs64, n = c.reference(np.float32)
    _, ost = c.oracle()
    bound = GR.hard_bound(n, abs64, sum64, U32, GR.atomic_adds(n)) + GR.ref_bound(n, abs64)
    worst, bad = GR.tier1(got, sum64, abs64, n, bound)
    st = GR.stats(GR.units(got, sum64, abs64, U32), n)
    failed = (["tier 1: %d elements, worst %.3g" % (bad, worst)] if bad else [])
    if not GR.within(st, ost):
        failed.append("tier 2: %s" % {k: round(v, 2) for k, v in GR.ratios(st, ost).items()})
    return failed


@pytest.mark.parametrize("mutant", list(MUTANTS))
@pytest.mark.parametrize("name", GR.MUTANT_CASES)
def test_mutants_pass_the_old_bar_and_fail_the_new(name, mutant):
    """The mutant's table gradient: the C oracle's (its real float32 accumulation error) plus what the mutation changes
    in the exact sum of the terms."""
    c = GR.case(name)
    sum64, abs64, n = c.reference(np.float32)
    ge, _ = c.oracle()
    msum, _, _ = GR.terms_reference(c.grad(np.float32), c.x, c.rows, c.offsets, c.S, c.H, c.gridtype, c.align, np.float32,
                                    **MUTANTS[mutant])
    got = (ge.astype(np.float64) + (msum - sum64)).astype(np.float32)
    assert not np.array_equal(got, ge), "the mutation changes nothing on this case"
    old_err = float(np.abs(got.astype(np.float64) - ge).max())
    old_bar = 1e-5 * max(1.0, float(np.abs(ge).max()))
    failed = _verdict(c, got)
    print("%s / %s: old bar %.2e of %.2e; new: %s" % (name, mutant, old_err, old_bar, failed))
    assert old_err <= old_bar, "this mutant is not subtle: the old bar sees it"
    assert failed, "the per-element bounds do not see this mutant"
    assert not _verdict(c, ge)   # and the unmutated result passes them


# --------------------------------------------------------------------------------------------------- edges of units
def test_units_edges():
    sum64 = np.array([[0.0, 0.0], [1.5, -2.0 ** -140], [3.0, 1.0]])
    abs64 = np.array([[0.0, 0.0], [1.5, 2.0 ** -140], [5.0, 1.0]])
    n = np.array([0, 1, 3])
    got = np.array([[0.0, -0.0], [1.5, -2.0 ** -140], [3.0 + 2.0 ** -22, 1.0]], np.float32)
    un = GR.units(got, sum64, abs64, U32)
    assert un[0].tolist() == [0.0, 0.0] and un[1].tolist() == [0.0, 0.0]          # untouched: zero of either sign
    assert un[2, 0] == pytest.approx(2.0 ** -22 / (U32 * 5.0)) and un[2, 1] == 0
    got[0, 1] = np.float32(2.0 ** -149)                                            # the smallest value there is
    assert GR.units(got, sum64, abs64, U32)[0, 1] == np.inf
    bound = GR.hard_bound(n, abs64, sum64, U32, GR.atomic_adds(n))
    assert bound[0].tolist() == [0.0, 0.0] and bound[1].tolist() == [0.0, 0.0]     # n <= 1: exact or nothing
    assert bound[2, 0] == pytest.approx(2 * U32 * 5.0, rel=1e-6)
    assert GR.tier1(got, sum64, abs64, n, bound) == (pytest.approx(2.0 ** -22 / bound[2, 0]), 1)   # [0, 1] is beyond its bound of 0
    # a non-zero starting table is one more addend of every element, and all there is of an untouched one
    old = np.array([[-0.0, 7.0], [1.0, 0.0], [-3.0, 2.0]], np.float32)
    s2, a2 = GR.with_start(sum64, abs64, old)
    assert s2[0].tolist() == [0.0, 7.0] and a2[0].tolist() == [0.0, 7.0] and a2[2].tolist() == [8.0, 3.0]
    keep = np.array([[-0.0, 7.0]], np.float32)
    assert GR.units(keep, s2[:1], a2[:1], U32).tolist() == [[0.0, 0.0]]
    assert GR.units(keep + np.float32(2.0 ** -20), s2[:1], a2[:1], U32)[0].tolist() == [np.inf, 2.0 ** -20 / (U32 * 7.0)]
    assert GR.stats(un, n) == dict(elements=2, median=pytest.approx(un[2, 0] / 2), p99=pytest.approx(un[2, 0] * 0.99),
                                   max=un[2, 0])
    assert GR.stats(un[:2], n[:2])["elements"] == 0
    # the store term, and adds capped by the reduce levels
    assert GR.hard_bound(np.array([1]), np.array([[2.0]]), np.array([[-2.0]]), U32, 0, 2.0 ** -11)[0, 0] == 2.0 ** -10
    assert GR.det_adds(np.array([0, 1, 2, 50, 5000]), 3 * 20000 * 4, False).tolist() == [0, 0, 1, 27, 27]
    assert GR.det_adds(np.array([0, 1, 2, 50, 5000]), 3 * 20000 * 4, True).tolist() == [1, 1, 2, 28, 28]
