"""float64 reference of variable-length packed-QKV attention, written for this repository.

qkv is binary16 [total, 3, H, d], cu_seqlens the segment bounds, dout binary16 [total, H, d].  Per segment and head,
from the binary16 values widened to double:

    P = softmax(scale Q K^T)   out = P V          dV = P^T dO     dP = dO V^T     D = rowsum(dO o out)
    dS = P o (dP - D)          dQ = scale dS K    dK = scale dS^T Q

With each result comes its SCALE, the same formula with every term replaced by its absolute value
(A_out = P |V|, A_dV = P^T |dO|, A_dS = P o (|dO| |V|^T + rowsum(|dO| o |out|)), A_dQ = |scale| A_dS |K|,
A_dK = |scale| A_dS^T |Q|), and a FLOOR for operands that fall into binary16's subnormal range (t = 2^-24, sums
over the segment's rows: F_out = t (sum|V| + 1), F_dV = t (sum|dO| + 1), F_dQ = |scale| t sum|K| + t,
F_dK = |scale| t sum|Q| + t).  One UNIT of an element is 2^-11 A + F; errors are reported in units.

emulate() is the same computation with the rounding contract of include/gca.h applied at exactly its rounding
points: fp32 scores, maximum, sum and log-sum-exp, binary16 P and dS as operands, binary16 results.
"""
import numpy as np

T_SUB = 2.0 ** -24
EPS_HALF = 2.0 ** -11
RAGGED_LENS = [1, 2, 15, 16, 17, 63, 64, 65, 333, 1023, 1024, 0, 5]
AMPLITUDES = [0.1, 1.0, 3.0, 6.0, 10.0]
NAMES = ("out", "dq", "dk", "dv")


def cu_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def random_case(seed, lens, heads, d=16, qk_amp=1.0, v_amp=1.0, do_amp=1.0, total=None):
    """rng.normal inputs rounded to binary16: (qkv [total, 3, H, d], cu_seqlens, dout [total, H, d])."""
    rng = np.random.default_rng(seed)
    cu = cu_of(lens)
    total = int(cu[-1]) if total is None else total
    qkv = rng.normal(size=(total, 3, heads, d))
    qkv[:, :2] *= qk_amp
    qkv[:, 2] *= v_amp
    dout = rng.normal(size=(total, heads, d)) * do_amp
    return qkv.astype(np.float16), cu, dout.astype(np.float16)


def segments(cu, total, max_seqlen=None):
    """(first row, length) of every segment, clamped as the library clamps."""
    cu = np.clip(np.asarray(cu, np.int64), 0, total)
    for s in range(len(cu) - 1):
        n = max(int(cu[s + 1] - cu[s]), 0)
        if max_seqlen is not None:
            n = min(n, int(max_seqlen))
        yield int(cu[s]), n


def _one(q, k, v, do, scale):
    s = scale * (q @ k.T)
    s -= s.max(axis=1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=1, keepdims=True)
    out = p @ v
    dv = p.T @ do
    dp = do @ v.T
    dd = (do * out).sum(axis=1, keepdims=True)
    ds = p * (dp - dd)
    dq = scale * (ds @ k)
    dk = scale * (ds.T @ q)
    a_out = p @ np.abs(v)
    a_dv = p.T @ np.abs(do)
    a_ds = p * (np.abs(do) @ np.abs(v).T + (np.abs(do) * np.abs(out)).sum(axis=1, keepdims=True))
    a_dq = abs(scale) * (a_ds @ np.abs(k))
    a_dk = abs(scale) * (a_ds.T @ np.abs(q))
    ones = np.ones((q.shape[0], 1))
    f_out = ones * (T_SUB * (np.abs(v).sum(axis=0) + 1.0))
    f_dv = ones * (T_SUB * (np.abs(do).sum(axis=0) + 1.0))
    f_dq = ones * (abs(scale) * T_SUB * np.abs(k).sum(axis=0) + T_SUB)
    f_dk = ones * (abs(scale) * T_SUB * np.abs(q).sum(axis=0) + T_SUB)
    val = (out, dq, dk, dv)
    unit = (EPS_HALF * a_out + f_out, EPS_HALF * a_dq + f_dq, EPS_HALF * a_dk + f_dk, EPS_HALF * a_dv + f_dv)
    return val, unit


def reference(qkv, cu, dout, scale=None, max_seqlen=None):
    """{'out', 'dq', 'dk', 'dv'} float64 [total, H, d] and the matching {'u_out', ...} units.  Rows that no segment
    covers are 0 with a unit of 0."""
    total, _, heads, d = qkv.shape
    scale = d ** -0.5 if scale is None else float(scale)
    x = qkv.astype(np.float64)
    g = dout.astype(np.float64)
    res = {n: np.zeros((total, heads, d)) for n in NAMES}
    res.update({"u_" + n: np.zeros((total, heads, d)) for n in NAMES})
    for b, n in segments(cu, total, max_seqlen):
        if n == 0:
            continue
        for h in range(heads):
            val, unit = _one(x[b:b + n, 0, h], x[b:b + n, 1, h], x[b:b + n, 2, h], g[b:b + n, h], scale)
            for name, a, u in zip(NAMES, val, unit):
                res[name][b:b + n, h] = a
                res["u_" + name][b:b + n, h] = u
    return res


def emulate(qkv, cu, dout, scale=None, max_seqlen=None):
    """The rounding contract on the CPU: {'out', 'dq', 'dk', 'dv'} binary16 [total, H, d]."""
    total, _, heads, d = qkv.shape
    scale = np.float32(d ** -0.5 if scale is None else scale)
    x = qkv.astype(np.float32)
    g = dout.astype(np.float32)
    res = {n: np.zeros((total, heads, d), np.float16) for n in NAMES}
    for b, n in segments(cu, total, max_seqlen):
        if n == 0:
            continue
        for h in range(heads):
            q, k, v, do = x[b:b + n, 0, h], x[b:b + n, 1, h], x[b:b + n, 2, h], g[b:b + n, h]
            s = (q @ k.T) * scale
            m = s.max(axis=1, keepdims=True)
            e = np.exp(s - m)
            l = e.sum(axis=1, keepdims=True, dtype=np.float32)
            lse = m + np.log(l)
            out = ((e.astype(np.float16).astype(np.float32) @ v) / l).astype(np.float16)
            p = np.exp(s - lse)
            p16 = p.astype(np.float16).astype(np.float32)
            dd = (do * out.astype(np.float32)).sum(axis=1, keepdims=True, dtype=np.float32)
            ds16 = (p * (do @ v.T - dd)).astype(np.float16).astype(np.float32)
            res["out"][b:b + n, h] = out
            res["dv"][b:b + n, h] = (p16.T @ do).astype(np.float16)
            res["dq"][b:b + n, h] = (scale * (ds16 @ k)).astype(np.float16)
            res["dk"][b:b + n, h] = (scale * (ds16.T @ q)).astype(np.float16)
    return res


def errors_in_units(got, ref):
    """Largest |got - ref| / unit per tensor over EVERY element; an element whose unit is 0 (a row that no segment
    covers) must be exactly 0 and otherwise counts as infinitely wrong."""
    worst = {}
    for n in NAMES:
        err = np.abs(np.asarray(got[n], np.float64) - ref[n])
        unit = ref["u_" + n]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(unit > 0, err / unit, np.where(err == 0, 0.0, np.inf))
        worst[n] = float(r.max()) if r.size else 0.0
    return worst
