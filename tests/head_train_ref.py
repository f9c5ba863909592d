"""What the tests of the head's output layers in a training step (gcm_head_train_*, modlinear.head_attrs / head_points14;
DESIGN.md section 17c) share: seeded cases, a transcription of the library's plan, one direct call of the two C entry points
on torch's memory (it returns the stored `pre`, takes a stream and can pre-fill every output and the workspace), and the
float64 reference of the backward with its bars.

Forward: the reference and the bar are modlinear_ref.head_reference's.  Backward: float64 from the float32 operands and the
STORED float32 pre (so the side of the clamp an element sits on is not in question), every element within

    dh_ni   1e-5 * sum_c |dv_nc W_ci|        dW_ci   1e-5 * sum_n |dv_nc h_ni|        db_c   1e-5 * sum_n |dv_nc|

plus one float32 unit of the value; no element is left out.  dv = dout * factor * s (1 - s) with s = sigmoid(pre), for
`scale` dout * factor where -1 <= pre <= 1, and 0 for a row whose group is negative; in the [N, 14] form dout is the key's
columns of dP, for `scale` times scales."""
import ctypes as C

import numpy as np
import torch

from modlinear_ref import BAR, HEAD_FACTORS

KINDS = ("xyz", "rgb", "scale", "opacity")
P14_AT = {"xyz": 0, "opacity": 3, "scale": 4, "rgb": 11}
PRE_AT = {"xyz": 0, "rgb": 3, "scale": 6, "opacity": 9}
MAX_RECORDS, FOLD_GROUPS = 1024, 16
PLAN_FIELDS = ("tiles", "tpb", "records", "groups", "per", "levels", "rec_floats", "key_floats")
# at I = 8: a short last tile and 14 fold groups of 3 records; and beyond 65 536 rows, where a row block walks two tiles
# (the last block one) and the last tile is short
N_GROUPS, N_TWO_TILES = 64 * 39 + 7, 65536 + 128 + 5


def channels(kind):
    return 1 if kind == "opacity" else 3


def plan(N, I):
    """gcm_head_train_plan, transcribed."""
    tiles = (N + 63) // 64
    tpb = max(1, -(-tiles // MAX_RECORDS))
    records = -(-tiles // tpb)
    per = max(1, -(-records // FOLD_GROUPS))
    groups = max(1, -(-records // per))
    rec = 3 * I + 4
    return {"tiles": tiles, "tpb": tpb, "records": records, "groups": groups, "per": per, "levels": 2 if groups > 1 else 1,
            "rec_floats": rec, "key_floats": (records * rec + 63) // 64 * 64}


def workspace_bytes(N, I, n_keys):
    return (plan(N, I)["key_floats"] * n_keys * 4 + 255) // 256 * 256


def library_plan(N, I):
    from gaussiancity_amd import _native_m as M
    buf = (C.c_int64 * 8)()
    assert M.lib().gcm_head_train_plan(N, I, buf) == 0
    return dict(zip(PLAN_FIELDS, buf))


def make_case(N, I, kinds, seed, bias=True, group="mixed"):
    """Inputs of one case.  group: None, "mixed" (about 8 % of the rows, at least one from 15 rows on, at -1; the others at
    0 .. 4) or "bare" (every row at -1).  The scale key's weights are three times as large, so the clamp is active on some
    elements and not on others, and from 15 rows on rows 1 and 2 are crafted so that its pre is exactly +1 and -1."""
    rng = np.random.default_rng(seed)
    c = {"N": N, "I": I, "kinds": tuple(kinds), "group": None, "keys": {}}
    if group == "mixed":
        g = rng.integers(0, 5, size=N)
        g[rng.random(N) < 0.08] = -1
        if N >= 15:
            g[rng.integers(3, N)] = -1
            g[1:3] = 2
        c["group"] = g.astype(np.int32)
    elif group == "bare":
        c["group"] = np.full(N, -1, np.int32)
    for kind in kinds:
        Cn = channels(kind)
        k = {"h": rng.normal(size=(N, I)), "w": rng.normal(size=(Cn, I)) / np.sqrt(I) * (3.0 if kind == "scale" else 1.0),
             "b": rng.normal(size=Cn) * 0.3 if bias else None, "factor": HEAD_FACTORS[kind], "dout": rng.normal(size=(N, Cn))}
        if kind == "scale" and N >= 15:  # pre = h_0 * w_c0 + b_c, every other term an exact zero
            k["w"][:, 0] = 0.5
            k["h"][1:3] = 0.0
            if bias:
                k["b"][:] = 0.5
                k["h"][1, 0], k["h"][2, 0] = 1.0, -3.0
            else:
                k["h"][1, 0], k["h"][2, 0] = 2.0, -2.0
        c["keys"][kind] = {n: v.astype(np.float32) if isinstance(v, np.ndarray) else v for n, v in k.items()}
    c["xyz"] = rng.normal(size=(N, 3)).astype(np.float32)
    c["scales"] = rng.uniform(0.2, 1.5, size=(N, 3)).astype(np.float32)
    c["dp"] = rng.normal(size=(N, 14)).astype(np.float32)
    return c


def _dev(dev, a, extra=0, fill=7.0):
    """a on the device; extra: as a view of rows `extra` elements further apart than they are wide."""
    t = torch.from_numpy(a).to(dev)
    if not extra:
        return t
    wide = torch.full((a.shape[0], a.shape[1] + extra), fill, device=dev, dtype=t.dtype)
    wide[:, :a.shape[1]] = t
    return wide[:, :a.shape[1]]


def run_raw(dev, c, packed_out=False, packed_grad=False, need=("dh", "dw", "db"), stream=None, nan_fill=False, h_extra=0,
            dp_extra=0):
    """One gcm_head_train_forward and one gcm_head_train_backward, called directly.  Returns float32 numpy arrays: pre,
    out.<kind> (or p14), dh.<kind>, dw.<kind>, db.<kind>.  nan_fill: every output, pre and the workspace hold NaN before
    the calls.  h_extra / dp_extra: h / dP with rows that many elements further apart."""
    from gaussiancity_amd import _native_m as M
    L = M.lib()
    N, I, kinds = c["N"], c["I"], c["kinds"]
    stream = stream or torch.cuda.current_stream()
    new = (lambda *shape: torch.full(shape, float("nan"), device=dev)) if nan_fill else (lambda *shape: torch.empty(shape, device=dev))
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.stream(stream):
        t = {}
        keys = (M.HeadKey * len(kinds))()
        for key, kind in zip(keys, kinds):
            k, Cn = c["keys"][kind], channels(kind)
            h, w = _dev(dev, k["h"], h_extra), _dev(dev, k["w"])
            b = None if k["b"] is None else _dev(dev, k["b"])
            t[kind] = {"h": h, "w": w, "b": b, "out": None if packed_out else new(N, Cn),
                       "dout": None if packed_grad else _dev(dev, k["dout"]),
                       "dh": new(N, I) if "dh" in need else None, "dw": new(Cn, I) if "dw" in need else None,
                       "db": new(Cn) if "db" in need and b is not None else None}
            key.kind, key.factor, key.h, key.h_stride, key.w, key.b = M.KINDS[kind], k["factor"], h.data_ptr(), h.stride(0) if N else I, w.data_ptr(), ptr(b)
            key.out, key.out_stride, key.dout, key.dout_stride = ptr(t[kind]["out"]), Cn, ptr(t[kind]["dout"]), Cn
            key.dh, key.dh_stride, key.dw, key.db = ptr(t[kind]["dh"]), I, ptr(t[kind]["dw"]), ptr(t[kind]["db"])
        group = None if c["group"] is None else torch.from_numpy(c["group"]).to(dev)
        pre = new(N, L.gcm_head_train_pre_floats())
        xyz, scales = _dev(dev, c["xyz"]), _dev(dev, c["scales"])
        p14 = new(N, 14) if packed_out else None
        dp = _dev(dev, c["dp"], dp_extra) if packed_grad else None
        nbytes = L.gcm_head_train_workspace_bytes(N, I, len(kinds))
        assert nbytes == workspace_bytes(N, I, len(kinds))
        work = torch.full((max(nbytes, 1) // 4 + 1,), float("nan"), device=dev) if nan_fill else torch.empty(max(nbytes, 1) // 4 + 1, device=dev)
        sp = C.c_void_p(stream.cuda_stream)
        M.check(L.gcm_head_train_forward(keys, len(kinds), ptr(group), N, I, pre.data_ptr(), xyz.data_ptr(), 3, scales.data_ptr(), 3,
                                         ptr(p14), sp), "gcm_head_train_forward")
        M.check(L.gcm_head_train_backward(keys, len(kinds), ptr(group), N, I, pre.data_ptr(), scales.data_ptr(), 3, ptr(dp),
                                          dp.stride(0) if packed_grad and N else 14, work.data_ptr(), nbytes, sp),
                "gcm_head_train_backward")
        stream.synchronize()
    res = {"pre": pre.cpu().numpy()}
    if packed_out:
        res["p14"] = p14.cpu().numpy()
    for kind in kinds:
        for name in ("out", "dh", "dw", "db"):
            if t[kind][name] is not None:
                res["%s.%s" % (name, kind)] = t[kind][name].cpu().numpy()
    return res


def dout_of(c, kind, packed_grad):
    """The key's incoming gradient in float64: its dout, or its columns of dP (times scales for `scale`)."""
    if not packed_grad:
        return c["keys"][kind]["dout"].astype(np.float64)
    d = c["dp"][:, P14_AT[kind]:P14_AT[kind] + channels(kind)].astype(np.float64)
    return d * c["scales"].astype(np.float64) if kind == "scale" else d


def reference(c, pre, packed_grad):
    """{name: (value, bar)} of dh.<kind>, dw.<kind>, db.<kind> in float64 from the stored pre, and {kind: dv}."""
    live = np.ones(c["N"], bool) if c["group"] is None else c["group"] >= 0
    ref, dvs = {}, {}
    for kind in c["kinds"]:
        k, Cn = c["keys"][kind], channels(kind)
        p = pre[:, PRE_AT[kind]:PRE_AT[kind] + Cn].astype(np.float64)
        d = dout_of(c, kind, packed_grad)
        if kind == "scale":
            slope = np.where((p >= -1) & (p <= 1), k["factor"], 0.0)
        else:
            s = 1.0 / (1.0 + np.exp(-p))
            slope = k["factor"] * s * (1 - s)
        dv = np.where(live[:, None], d * slope, 0.0)
        h, w = k["h"].astype(np.float64), k["w"].astype(np.float64)
        unit = lambda v: np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)  # noqa: E731
        for name, val, mag in (("dh", dv @ w, np.abs(dv) @ np.abs(w)), ("dw", dv.T @ h, np.abs(dv).T @ np.abs(h)),
                               ("db", dv.sum(0), np.abs(dv).sum(0))):
            ref["%s.%s" % (name, kind)] = (val, BAR * mag + unit(val))
        dvs[kind] = dv
    return ref, dvs


def hold(c, got, pre, packed_grad, label):
    """Every gradient in got (dh.<kind>, dw.<kind>, db.<kind>) within its bar; rows of a negative group exact zeros of dh."""
    ref, dvs = reference(c, pre, packed_grad)
    bad = []
    for name, g in got.items():
        if name.split(".")[0] not in ("dh", "dw", "db"):
            continue
        val, bar = ref[name]
        assert g.shape == val.shape, (name, g.shape, val.shape)
        err = np.abs(g.astype(np.float64) - val)
        print("%s %-10s worst error %.2e of its bar" % (label, name, float((err / bar).max()) if err.size else 0.0))
        if not (err <= bar).all():
            bad.append((name, float((err / bar).max()), int((err > bar).sum())))
        if name.startswith("dh.") and c["group"] is not None:
            assert not g[c["group"] < 0].any(), name
    assert not bad, bad
    return dvs
