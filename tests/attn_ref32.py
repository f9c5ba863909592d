"""float32 companion of tests/attn_ref.py: inputs, units and two float32 formulations of
variable-length packed-QKV attention for the float32 kernels of libgca_hip.so.

The float64 values come from attn_ref.reference, which widens whatever it is given.  The SCALES A are attn_ref's
(A_out = P |V|, A_dV = P^T |dO|, A_dS = P o (|dO| |V|^T + rowsum(|dO| o |out|)), A_dQ = |scale| A_dS |K|,
A_dK = |scale| A_dS^T |Q|), computed here.  One FLOAT32 UNIT of an element is

    2^-24 (1 + Smax) A        Smax = the largest |scale q . k| of the element's (segment, head), in float64

because a score is known to 2^-24 of its magnitude at best, and an absolute error e of a score is a relative error e
of its probability.  There is no floor: float32 inputs of these amplitudes stay far from the subnormal range.

  emulate32   the contract of include/gca.h in numpy float32: log-sum-exp form, P recomputed from it in the backward,
              D = rowsum(dO o out) from the stored out
  torch32     the backbone's non-flash formulation, (q * scale) @ k^T, softmax, @ v, in torch float32 with autograd, on
              any device: the yardstick that the kernels are held to
"""
import numpy as np

import attn_ref as R

EPS32 = 2.0 ** -24
NAMES = R.NAMES
QK_AMPS = [0.1, 1.0, 3.0, 6.0]  # at 10 probabilities underflow in binary32 and the torch formulation itself breaks


def random_case32(seed, lens, heads, d=16, qk_amp=1.0, v_amp=1.0, do_amp=1.0, total=None):
    """rng.normal inputs in float32: (qkv [total, 3, H, d], cu_seqlens, dout [total, H, d])."""
    rng = np.random.default_rng(seed)
    cu = R.cu_of(lens)
    total = int(cu[-1]) if total is None else total
    qkv = rng.normal(size=(total, 3, heads, d))
    qkv[:, :2] *= qk_amp
    qkv[:, 2] *= v_amp
    dout = rng.normal(size=(total, heads, d)) * do_amp
    return qkv.astype(np.float32), cu, dout.astype(np.float32)


def _units(q, k, v, do, scale):
    s = scale * (q @ k.T)
    smax = np.abs(s).max()
    s -= s.max(axis=1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=1, keepdims=True)
    out = p @ v
    a_out = p @ np.abs(v)
    a_dv = p.T @ np.abs(do)
    a_ds = p * (np.abs(do) @ np.abs(v).T + (np.abs(do) * np.abs(out)).sum(axis=1, keepdims=True))
    a_dq = abs(scale) * (a_ds @ np.abs(k))
    a_dk = abs(scale) * (a_ds.T @ np.abs(q))
    f = EPS32 * (1.0 + smax)
    return (f * a_out, f * a_dq, f * a_dk, f * a_dv), smax


def reference32(qkv, cu, dout, scale=None, max_seqlen=None):
    """attn_ref.reference's float64 values with float32 units under 'u_out' ...; 'smax' is the largest Smax."""
    total, _, heads, d = qkv.shape
    res = R.reference(qkv, cu, dout, scale, max_seqlen)
    scale = d ** -0.5 if scale is None else float(scale)
    x, g = qkv.astype(np.float64), dout.astype(np.float64)
    for n in NAMES:
        res["u_" + n] = np.zeros((total, heads, d))
    res["smax"] = 0.0
    for b, n in R.segments(cu, total, max_seqlen):
        for h in range(heads if n else 0):
            unit, smax = _units(x[b:b + n, 0, h], x[b:b + n, 1, h], x[b:b + n, 2, h], g[b:b + n, h], scale)
            res["smax"] = max(res["smax"], float(smax))
            for name, u in zip(NAMES, unit):
                res["u_" + name][b:b + n, h] = u
    return res


def emulate32(qkv, cu, dout, scale=None, max_seqlen=None):
    """The float32 contract on the CPU: {'out', 'dq', 'dk', 'dv'} float32 [total, H, d]."""
    total, _, heads, d = qkv.shape
    scale = np.float32(d ** -0.5 if scale is None else scale)
    x, g = qkv.astype(np.float32), dout.astype(np.float32)
    res = {n: np.zeros((total, heads, d), np.float32) for n in NAMES}
    for b, n in R.segments(cu, total, max_seqlen):
        for h in range(heads if n else 0):
            q, k, v, do = x[b:b + n, 0, h], x[b:b + n, 1, h], x[b:b + n, 2, h], g[b:b + n, h]
            s = (q @ k.T) * scale
            m = s.max(axis=1, keepdims=True)
            e = np.exp(s - m)
            l = e.sum(axis=1, keepdims=True, dtype=np.float32)
            lse = m + np.log(l)
            out = (e @ v) / l
            p = np.exp(s - lse)
            dd = (do * out).sum(axis=1, keepdims=True, dtype=np.float32)
            ds = p * (do @ v.T - dd)
            res["out"][b:b + n, h] = out
            res["dv"][b:b + n, h] = p.T @ do
            res["dq"][b:b + n, h] = scale * (ds @ k)
            res["dk"][b:b + n, h] = scale * (ds.T @ q)
    return res


def torch32(qkv, cu, dout, scale=None, max_seqlen=None, device="cpu"):
    """The non-flash branch's formulation in torch float32 with autograd on `device`, segment by segment."""
    import torch
    total, _, heads, d = qkv.shape
    scale = d ** -0.5 if scale is None else float(scale)
    x = torch.from_numpy(np.ascontiguousarray(qkv, np.float32)).to(device)
    g = torch.from_numpy(np.ascontiguousarray(dout, np.float32)).to(device)
    res = {n: np.zeros((total, heads, d), np.float32) for n in NAMES}
    for b, n in R.segments(cu, total, max_seqlen):
        if n == 0:
            continue
        q, k, v = (x[b:b + n, i].transpose(0, 1).contiguous().requires_grad_(True) for i in range(3))  # [H, n, d]
        attn = torch.softmax((q * scale) @ k.transpose(-2, -1), dim=-1)
        out = attn @ v
        out.backward(g[b:b + n].transpose(0, 1))
        for name, t in zip(NAMES, (out.detach(), q.grad, k.grad, v.grad)):
            res[name][b:b + n] = t.transpose(0, 1).cpu().numpy()
    return res


def errors_in_units(got, ref):
    return R.errors_in_units(got, ref)


def worst_of(rows):
    """Per tensor, the largest figure over a list of errors_in_units results."""
    return {n: max(r[n] for r in rows) for n in NAMES}


# ---- the input set of the float32 checks (tests/test_attention32_host.py, tests/test_attention32_gpu.py): ragged lengths
# at every head dimension, score amplitudes up to Smax of a few hundred, unbalanced V / dO, several key blocks with a
# moving maximum, and a max_seqlen cut.  (name, lens, heads, d, random_case32 keywords, max_seqlen)
INPUT_SET = (
    [("ragged d16", R.RAGGED_LENS, 2, 16, {}, None)]
    + [("ragged d%d" % d, [1, 17, 64, 65, 333], 2, d, {}, None) for d in (32, 64)]
    + [("qk_amp %g" % a, [300, 64], 2, 16, {"qk_amp": a}, None) for a in QK_AMPS]
    + [("v_amp 100, do_amp 0.01", [257, 16], 2, 16, {"v_amp": 100.0, "do_amp": 0.01}, None),
       ("one segment of 1300", [1300], 2, 16, {}, 1300),
       ("cut at 100", [257], 2, 16, {}, 100)])
_CASES = {}


def input_case(i):
    """(name, qkv, cu, dout, max_seqlen, reference32) of INPUT_SET[i]; computed once per process, never modified."""
    if i not in _CASES:
        name, lens, heads, d, kw, cut = INPUT_SET[i]
        qkv, cu, dout = random_case32(3200 + i, lens, heads, d, **kw)
        _CASES[i] = (name, qkv, cu, dout, cut, reference32(qkv, cu, dout, None, cut))
    return _CASES[i]
