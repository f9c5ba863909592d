"""The hash-grid encoder's table gradient, element by element -- shared by the host tests (test_grid_rows_host.py), the
GPU tests (test_grid_rows_gpu.py) and tools/grid_rows.py.  numpy only at import; nothing here needs a GPU but gpu_backward.

grad_embeddings[row][ch] is a sum of terms w * g, one per (level, point, corner) whose corner lands on the row.  The
suite's older bar for it is one scalar per table, max|d| <= 1e-5 * max(1, max|ref|) (2e-2 in binary16, 1e-12 in double):
the few rows with thousands of contributions decide it, and a row of a 2^19-row level that five points touch is not seen
at all.  Here every element is held to what summing ITS OWN terms in the kernel's number format can cost:

    terms_reference   the addends exactly as the kernels form them (float32 weight chain, cell and in-range decision on
                      the float32 bits, GceOps<T>::mulw for the product), summed without rounding worth speaking of:
                      sum64 = sum t, abs64 = sum |t|, n = number of contributions of the row.
    hard_bound        tier 1: ((1 + u_acc)^adds - 1) * abs64 + u_store * |sum64|, the classical bound of ANY summation
                      order in which no term passes through more than `adds` roundings (Higham, Accuracy and Stability,
                      section 4.2), plus one rounding of the stored value where the store narrows.  adds comes from
                      reading the kernel (atomic_adds / det_adds), never from what it returned.
    units, stats      tier 2: |got - sum64| / (u * abs64) per element; its median, 99th percentile and maximum over the
                      elements with n >= 2 are compared with what the C oracle (a sequential float32 sum of the same
                      terms) leaves on the same case -- `M` = 4 times that, tests/grad_rows.py's factor, for the same
                      reason: the summation order differs, the arithmetic does not.
"""
import functools
import math

import numpy as np

import grid_util as GU
from oracle import grid_oracle_typed as GT

M = 4.0
STATS = ("median", "p99", "max")
U = {np.float16: 2.0 ** -11, np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
DET_TILE = 256   # entries per k_det_reduce workgroup (gce_det.h)


# ------------------------------------------------------------------------------------------------ reference
def _contributions(inputs, offsets, S, H, gridtype, align_corners):
    """Yields (level, points, rows, w) for every corner of every level: the in-range points, the global table row their
    corner lands on and the float32 weight -- grid_oracle_typed.backward's loop, rows instead of element indices."""
    x = np.ascontiguousarray(inputs, np.float32)
    D, L = x.shape[1], len(offsets) - 1
    sc = GT.level_scales(L, S, H)
    one = np.float32(1.0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for l in range(L):
            hs = int(offsets[l + 1] - offsets[l])
            res = int(np.ceil(sc[l])) + 1
            inside, pos, pg = GT._locate(x, sc[l], align_corners)
            pts = np.flatnonzero(inside)
            for idx in range(1 << D):
                w = np.ones(len(x), np.float32)
                pl = pg.copy()
                for d in range(D):
                    if idx & (1 << d):
                        w = (w * pos[:, d]).astype(np.float32)
                        pl[:, d] = pg[:, d] + np.uint32(1)
                    else:
                        w = (w * (one - pos[:, d])).astype(np.float32)
                rows = GT._grid_index(gridtype, align_corners, hs, res, pl, 1) + int(offsets[l])
                yield l, pts, rows[pts], w[pts]


def _mulw(w, g, T):
    """GceOps<T>::mulw in IEEE arithmetic, subnormals kept; the result as float64 (exact for all three)."""
    if T == np.float32:
        return (w[:, None] * g).astype(np.float32).astype(np.float64)
    return GT._mulw(w[:, None], g, T).astype(np.float64)


def terms_reference(grad, inputs, total_rows, offsets, S, H, gridtype, align_corners, dtype, weight_fn=None,
                    term_fn=None):
    """grad [L,B,C] -> (sum64 [rows,C], abs64 [rows,C], n [rows]).  dtype: np.float16 / float32 / float64, the kernels'
    scalar_t; grad is taken in that dtype.  In float16 and float32 the terms have at most 24 significant bits and the
    float64 sums (one np.bincount per channel) are 2^29 times finer than the kernels'; in float64 the terms have up to
    77 bits, so they are summed in numpy's longdouble and sum64 / abs64 come back as longdouble.  ref_bound says what
    either leaves.  weight_fn(w) -> (w', keep mask) and term_fn(t) -> t' alter the weights, drop corners and alter the
    terms: the host tests' mutants, never used by a reference."""
    T = np.dtype(dtype).type
    g_all = np.ascontiguousarray(grad, T)
    C = g_all.shape[2]
    rows_l, terms_l = [], []
    with np.errstate(under="ignore"):
        for l, pts, rows, w in _contributions(inputs, offsets, S, H, gridtype, align_corners):
            if weight_fn is not None:
                w, keep = weight_fn(w)
                pts, rows, w = pts[keep], rows[keep], w[keep]
            t = _mulw(w, g_all[l][pts], T)
            if term_fn is not None:
                t = term_fn(t)
            rows_l.append(rows)
            terms_l.append(t)
    rows = np.concatenate(rows_l) if rows_l else np.zeros(0, np.int64)
    terms = np.concatenate(terms_l) if terms_l else np.zeros((0, C))
    assert rows.size == 0 or (0 <= int(rows.min()) and int(rows.max()) < total_rows)
    n = np.bincount(rows, minlength=total_rows).astype(np.int64)
    if T == np.float64:
        acc = np.longdouble
        sum64, abs64 = np.zeros((total_rows, C), acc), np.zeros((total_rows, C), acc)
        if rows.size:
            order = np.argsort(rows, kind="stable")
            sr = rows[order]
            starts = np.flatnonzero(np.r_[True, sr[1:] != sr[:-1]])
            tl = terms[order].astype(acc)
            sum64[sr[starts]] = np.add.reduceat(tl, starts, axis=0)
            abs64[sr[starts]] = np.add.reduceat(np.abs(tl), starts, axis=0)
    else:
        sum64, abs64 = np.empty((total_rows, C)), np.empty((total_rows, C))
        for ch in range(C):
            sum64[:, ch] = np.bincount(rows, weights=terms[:, ch], minlength=total_rows)
            abs64[:, ch] = np.bincount(rows, weights=np.abs(terms[:, ch]), minlength=total_rows)
    return sum64, abs64, n


def ref_bound(n, abs64):
    """What the reference's own accumulation (sequential, in abs64's format) can be off by: for the longdouble sums of
    the double path 2^-11 of the kernel's bound, for the float64 sums of 24-bit terms nothing that matters."""
    u = float(np.finfo(abs64.dtype).eps) / 2
    return np.expm1(np.maximum(n - 1, 0)[:, None] * math.log1p(u)) * abs64


def with_start(sum64, abs64, old):
    """The sums of a pass that adds into a table that held `old`: old is one more addend of every element."""
    o = old.astype(sum64.dtype)
    return sum64 + o, abs64 + np.abs(o)


# ------------------------------------------------------------------------------------------------ statistic and bound
def units(got, sum64, abs64, u):
    """|got - sum64| / (u * abs64) per element: 0 where both are zero, inf where abs64 == 0 and got != 0 (an element
    nobody contributes to, or whose terms are all zero, must be an exact zero)."""
    err = np.abs(got.astype(sum64.dtype) - sum64).astype(np.float64)
    den = u * abs64.astype(np.float64)
    out = np.zeros(err.shape)
    np.divide(err, den, out=out, where=den > 0)
    out[(den == 0) & (err > 0)] = np.inf
    return out


def hard_bound(n, abs64, sum64, u_acc, adds, u_store=0.0):
    """((1 + u_acc)^adds - 1) * abs64 + u_store * |sum64|; adds: scalar or [rows] (broadcast over the channels), n: [rows]
    (an element with n == 0 gets the bound 0 whatever adds says)."""
    adds = np.where(n > 0, np.broadcast_to(np.asarray(adds, np.float64), n.shape), 0.0)[:, None]
    return (np.expm1(adds * math.log1p(u_acc)) * abs64 + u_store * np.abs(sum64)).astype(np.float64)


def atomic_adds(n):
    """k_grid_bwd / k_grid_bwd_t: one atomic add per term into a zeroed element.  The first is 0 + t, exact; every later
    one rounds once, whatever the order: no term passes through more than n - 1 roundings."""
    return np.maximum(n - 1, 0)


def det_levels(contributions):
    """Reduce levels of gce_backward_det for L * B * 2^D contributions: det_layout's recurrence."""
    levels, c = 1, int(contributions)
    while c > DET_TILE:
        c = 2 * ((c + DET_TILE - 1) // DET_TILE)
        levels += 1
    return levels


def det_adds(n, contributions, nonzero_start):
    """k_det_reduce (derivation in test_grid_rows_gpu.py's docstring): at most 9 additions on any term's way per reduce
    level; every addition joins two non-empty partial sums of the row, so n - 1 at most however many levels; the
    closing old + sum is exact into a zeroed table and one more rounding otherwise."""
    return np.minimum(np.maximum(n - 1, 0), 9 * det_levels(contributions)) + (1 if nonzero_start else 0)


def stats(un, n):
    """median / p99 / max of the units over the elements with n >= 2 (n == 1 is exact on every path: tier 1)."""
    v = un[n >= 2].reshape(-1)
    if v.size == 0:
        return dict(elements=0, median=0.0, p99=0.0, max=0.0)
    return dict(elements=int(v.size), median=float(np.median(v)), p99=float(np.percentile(v, 99)), max=float(v.max()))


def within(st, oracle_st, limits=None):
    """Every statistic within its limit (M, or limits[name]) times the oracle's.  Where the oracle's is 0 the limit is
    M units: one rounding of a two-term sum is already 1."""
    limits = limits or {}
    return all(st[k] <= limits.get(k, M) * (oracle_st[k] if oracle_st[k] > 0 else 1.0) for k in STATS)


def ratios(st, oracle_st):
    return {k: (st[k] / oracle_st[k] if oracle_st[k] > 0 else (0.0 if st[k] == 0 else float("inf"))) for k in STATS}


def tier1(got, sum64, abs64, n, bound):
    """-> (worst |got - sum64| / bound over the elements with a bound > 0, number of elements beyond their bound)."""
    err = np.abs(got.astype(sum64.dtype) - sum64).astype(np.float64)
    bad = int((err > bound).sum())
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    return worst, bad


# ------------------------------------------------------------------------------------------------ cases
# name -> (B, D, C, L, base, desired, log2_hashmap, gridtype, align_corners, seed, tiny).  The smallest shapes that reach
# each mechanism:
#   A  mixed: lists from 1 to about 2 700, 1 - 17 % of the rows with one contribution, points out of range and on both
#      closed ends;  B  GaussianCity's level shape, 2 097 152 rows, at most a handful of contributions each;
#   C  16 / 32 / 88 rows under 20 000 points: lists up to 18 001, runs across many 256-entry tiles, every record level;
#   D  ragged ends of the 256-entry tile;  E  A's D = 5 and D = 3 shapes with align_corners and a quarter of the points
#      moved to 2^-20, 1 - 2^-20 or 2^-30 in one to D coordinates: weights down to the float32 subnormals, binary16 terms
#      subnormal or zero.
CASES = {
    "A-d2": (3001, 2, 1, 5, 3, 50, 9, 0, False, 201, False),
    "A-d3": (3001, 3, 4, 5, 3, 50, 13, 1, True, 304, False),
    "A-d4": (3001, 4, 2, 5, 3, 50, 10, 0, True, 402, False),
    "A-d5": (3001, 5, 8, 5, 3, 50, 13, 0, False, 508, False),
    "B": (2048, 5, 8, 4, 16, 128, 19, 0, False, 19, False),
    "C-c8": (20000, 2, 8, 3, 2, 8, 10, 1, False, 39, False),
    "C-c1": (20000, 2, 1, 3, 2, 8, 10, 0, False, 32, False),
    "D-1": (1, 3, 2, 2, 3, 9, 9, 0, False, 1, False),
    "D-255": (255, 3, 2, 2, 3, 9, 9, 0, False, 255, False),
    "D-256": (256, 3, 2, 2, 3, 9, 9, 0, False, 256, False),
    "D-257": (257, 3, 2, 2, 3, 9, 9, 0, False, 257, False),
    "E-d5": (3001, 5, 8, 5, 3, 50, 13, 0, True, 558, True),
    "E-d3": (3001, 3, 4, 5, 3, 50, 13, 1, True, 354, True),
}
F32_CASES = tuple(CASES)
F64_CASES = ("A-d3", "A-d5", "E-d5", "E-d3")
F16_CASES = ("A-d3", "A-d5", "E-d5", "E-d3")
F16_DET_CASES = F16_CASES + ("B",)
MUTANT_CASES = ("A-d3", "A-d5", "B")


class Case:
    def __init__(self, name):
        (B, D, C, L, base, desired, lh, gridtype, align, seed, tiny) = CASES[name]
        rng = np.random.default_rng(seed)
        x, emb, offsets, S, H = GU.make_case(rng, B, D, C, L, base=base, desired=desired, log2_hashmap=lh,
                                             align_corners=align)
        if tiny:
            pick = rng.choice(B, B // 4, replace=False)
            vals = np.array([2.0 ** -20, 1.0 - 2.0 ** -20, 2.0 ** -30], np.float32)
            for b in pick:
                dims = rng.choice(D, int(rng.integers(1, D + 1)), replace=False)
                x[b, dims] = rng.choice(vals, len(dims))
        self.name, self.B, self.D, self.C, self.L = name, B, D, C, L
        self.x, self.offsets, self.S, self.H = x, offsets, S, H
        self.gridtype, self.align, self.rows = gridtype, align, int(offsets[-1])
        self.contributions = L * B * (1 << D)
        g64 = rng.normal(size=(L, B, C))
        self.grads = {np.float32: g64.astype(np.float32), np.float16: g64.astype(np.float16), np.float64: g64}
        self.table0 = rng.normal(size=(self.rows, C)).astype(np.float32)   # a non-zero starting table with -0.0 entries
        self.table0[::3] = -0.0
        self._ref, self._oracle = {}, None

    def grad(self, dtype):
        return self.grads[np.dtype(dtype).type]

    def reference(self, dtype):
        """(sum64, abs64, n) of this case in `dtype`; computed once, never written to."""
        T = np.dtype(dtype).type
        if T not in self._ref:
            r = terms_reference(self.grads[T], self.x, self.rows, self.offsets, self.S, self.H, self.gridtype, self.align, T)
            for a in r:
                a.setflags(write=False)
            self._ref[T] = r
        return self._ref[T]

    def oracle(self):
        """The C oracle's float32 table gradient (sequential sum in id order) and its tier-2 statistic."""
        if self._oracle is None:
            from oracle import grid_oracle as GO
            ge, _ = GO.backward(self.grads[np.float32], self.x, (self.rows, self.C), self.offsets, self.S, self.H, None,
                                self.gridtype, self.align)
            sum64, abs64, n = self.reference(np.float32)
            ge.setflags(write=False)
            self._oracle = (ge, stats(units(ge, sum64, abs64, U[np.float32]), n))
        return self._oracle


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ------------------------------------------------------------------------------------------------ the six paths
PATHS = ("atomic", "det")


def path_bound(c, path, dtype, nonzero_start=False):
    """(sum, abs, n, tier-1 bound) of case c on a path; with nonzero_start the table held c.table0 (in dtype) before."""
    T = np.dtype(dtype).type
    sum64, abs64, n = c.reference(T)
    if nonzero_start:
        sum64, abs64 = with_start(sum64, abs64, c.table0.astype(T))
    if path == "atomic":
        assert not nonzero_start
        u_acc, adds, u_store = U[T], atomic_adds(n), 0.0
    else:
        u_acc = U[np.float64] if T == np.float64 else U[np.float32]   # DetAcc: float for float32 and binary16 tables
        adds, u_store = det_adds(n, c.contributions, nonzero_start), (U[T] if T == np.float16 else 0.0)
    bound = hard_bound(n, abs64, sum64, u_acc, adds, u_store) + ref_bound(n + (1 if nonzero_start else 0), abs64)
    if nonzero_start:
        # an untouched element keeps its value (bound 0); a touched one is rounded once more as old + sum
        bound = np.where((n > 0)[:, None], bound + u_acc * np.abs(sum64).astype(np.float64), 0.0)
    return sum64, abs64, n, bound


def gpu_backward(c, path, dtype, dev, table0=None):
    """One table-gradient pass of case c on the GPU through ext_backward / ext_backward_deterministic -> numpy."""
    import torch
    from gaussiancity_amd import grid_encoder as GE
    T = np.dtype(dtype).type
    tdt = {np.float16: torch.float16, np.float32: torch.float32, np.float64: torch.float64}[T]
    x, off, grad = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (c.x, c.offsets, c.grad(T)))
    table = torch.zeros(c.rows, c.C, device=dev, dtype=tdt)
    ge = torch.zeros_like(table) if table0 is None else torch.from_numpy(table0.astype(T)).to(dev)
    dd, gi = torch.empty(1, device=dev, dtype=tdt), torch.zeros(1, device=dev, dtype=tdt)
    args = (grad, x, table, off, ge, c.B, c.D, c.C, c.L, c.S, c.H, False, dd, gi, c.gridtype, c.align)
    before = GE.stats()
    (GE.ext_backward_deterministic if path == "det" else GE.ext_backward)(*args)
    took = {k: v - before[k] for k, v in GE.stats().items()}
    assert took == {"atomic_backward_calls": int(path != "det"), "deterministic_backward_calls": int(path == "det")}, took
    return ge.cpu().numpy()
