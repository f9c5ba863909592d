"""What the GPU tests of the grouped modulated linear layer (gcm_modlinear_*, gcm_head_out) share:
seeded cases, the float64 numpy reference with the sum of absolute terms of every element, one forward + backward
through gaussiancity_amd.modlinear, and the bar.

The bar is tests/test_sparse_gpu.py's: every element within 1e-5 * (the sum of the absolute values of its terms) of the
float64 evaluation -- about a hundred times what a float32 fmaf chain of these lengths loses, and zero where an element
has no term at all (rows without a group, empty groups: those must be exact zeros).  The terms:

    y        sum_i |x_i a_i W_oi| + |beta_o| + |b_o|              dW_oi    sum_r |dpre_ro x_ri a_i|
    dx_i     |a_i| sum_o |dpre_o W_oi|                            dalpha_gi  sum_{r in g} |x_ri| sum_o |dpre_ro W_oi|
    dbeta_go, dbias_o    sum |dpre_ro|

dpre = dy * (y > 0 ? 1 : slope) is the header's rule on the STORED y, so the reference takes the sign from the y the
forward stored (an element whose float64 value is within rounding of 0 has no sign to agree on)."""
import numpy as np
import torch

BAR = 1e-5
LEAVES = ("x", "w", "alpha", "beta", "bias")            # the five differentiable inputs
GRADS = {"x": "dx", "w": "dw", "alpha": "dalpha", "beta": "dbeta", "bias": "dbias"}


def make_case(N, I, O, G, slope, bias, seed, plain=False):
    """Inputs of one case.  Rows of the groups interleaved at random; about 5 % of the rows (at least one from 20 rows
    on) are at -1.  G <= 5: group 3 has no rows.  G > 5: the groups g % 7 == 3 have no rows, the groups g % 7 == 5 have
    exactly one row each (as far as a quarter of the rows goes; the rest of them are empty too), and the other groups
    share the remaining rows at random.  plain: alpha, beta and group absent."""
    rng = np.random.default_rng(seed)
    c = {"x": rng.normal(size=(N, I)), "w": rng.normal(size=(O, I)) / np.sqrt(I), "dy": rng.normal(size=(N, O)),
         "alpha": None, "beta": None, "group": None, "bias": rng.normal(size=O) if bias else None, "slope": slope, "G": G}
    if not plain:
        c["alpha"], c["beta"] = 1.0 + 0.5 * rng.normal(size=(G, I)), rng.normal(size=(G, O))
        if G <= 5:
            group = rng.choice([g for g in range(G) if g != 3], size=N)
            group[rng.random(N) < 0.05] = -1
            if N >= 20:
                group[rng.integers(0, N)] = -1
        else:
            group = rng.choice([g for g in range(G) if g % 7 not in (3, 5)], size=N)
            bare = rng.random(N) < 0.05
            bare[rng.integers(0, N)] = True
            group[bare] = -1
            single = [g for g in range(G) if g % 7 == 5][:N // 4]
            group[rng.choice(np.flatnonzero(~bare), size=len(single), replace=False)] = single
        c["group"] = group.astype(np.int32)
    return {k: v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v for k, v in c.items()}


def reference(c, y_stored):
    """float64 values and the sums of absolute terms of y and the five gradients.  A group value outside 0 .. G-1 is a
    row without a group."""
    x, w, dy = (c[k].astype(np.float64) for k in ("x", "w", "dy"))
    (N, I), O, G, slope = x.shape, w.shape[0], c["G"], c["slope"]
    group = c["group"] if c["group"] is not None else np.zeros(N, np.int32)
    group = np.where((group >= 0) & (group < G), group, -1)
    live = (group >= 0)[:, None]
    gi = np.maximum(group, 0)
    a = c["alpha"].astype(np.float64)[gi] if c["alpha"] is not None else np.ones((N, I))
    be = c["beta"].astype(np.float64)[gi] if c["beta"] is not None else np.zeros((N, O))
    b = c["bias"].astype(np.float64) if c["bias"] is not None else np.zeros(O)
    xa = x * a * live
    pre = xa @ w.T + be + b
    val = {"y": np.where(pre > 0, pre, pre * slope) * live}
    mag = {"y": (np.abs(xa) @ np.abs(w).T + np.abs(be) + np.abs(b)) * live}
    dpre = dy * np.where(y_stored > 0, 1.0, slope) * live
    reach = np.abs(dpre) @ np.abs(w)            # sum_o |dpre_ro W_oi|
    dxs = dpre @ w
    val["dx"], mag["dx"] = dxs * a * live, np.abs(a) * reach * live
    val["dw"], mag["dw"] = dpre.T @ xa, np.abs(dpre).T @ np.abs(xa)
    onehot = (group[:, None] == np.arange(G)[None]).astype(np.float64)      # [N, G]
    val["dalpha"], mag["dalpha"] = onehot.T @ (dxs * x), onehot.T @ (np.abs(x) * reach)
    val["dbeta"], mag["dbeta"] = onehot.T @ dpre, onehot.T @ np.abs(dpre)
    val["dbias"], mag["dbias"] = dpre.sum(0), np.abs(dpre).sum(0)
    return val, mag


def _wide(t, extra, fill):
    """t [rows, width] as a view of rows `extra` elements further apart than they are wide, `fill` between them."""
    rows, width = t.shape
    wide = torch.full((rows, width + extra), fill, device=t.device, dtype=t.dtype)
    wide[:, :width] = t.detach()
    view = wide[:, :width]
    assert rows == 0 or (view.stride(0) == width + extra and (rows == 1 or not view.is_contiguous()))
    return view


def run(dev, c, strided=False, need=LEAVES, strided_w=False, strided_dy=False):
    """Forward + one backward through modulated_linear; y and the gradients as float32 numpy arrays.  strided /
    strided_w / strided_dy: x / weight / dy as views of rows 8 elements further apart than they are wide.  need: the
    leaves (of LEAVES) that require a gradient; a leaf the case does not have is skipped, and the gradient of a leaf
    that has none must be None and is left out of the result."""
    from gaussiancity_amd.modlinear import modulated_linear
    need = [k for k in need if c[k] is not None]
    assert need and set(need) <= set(LEAVES), need
    t = {k: None if c[k] is None else torch.from_numpy(c[k]).to(dev).requires_grad_(k in need) for k in LEAVES}
    if strided:
        t["x"] = _wide(t["x"], 8, 0.0).requires_grad_("x" in need)
    if strided_w:
        t["w"] = _wide(t["w"], 8, 7.0).requires_grad_("w" in need)
    group = None if c["group"] is None else torch.from_numpy(c["group"]).to(dev)
    y = modulated_linear(t["x"], t["w"], t["alpha"], t["beta"], t["bias"], group, c["slope"])
    assert y.dtype == torch.float32 and tuple(y.shape) == (c["x"].shape[0], c["w"].shape[0])
    dy = torch.from_numpy(c["dy"]).to(dev)
    if strided_dy:
        dy, seen = _wide(dy, 8, 7.0), []
        y.register_hook(lambda g: seen.append(g.stride()))
    y.backward(dy)
    assert not strided_dy or seen == [dy.stride()], "autograd handed the backward another dy than the strided one"
    res = {"y": y.detach().cpu().numpy()}
    for k in LEAVES:
        if t[k] is None:
            continue
        if k not in need:
            assert t[k].grad is None, GRADS[k]
            continue
        assert t[k].grad is not None and t[k].grad.shape == t[k].shape, GRADS[k]
        res[GRADS[k]] = t[k].grad.cpu().numpy()
    return res


def hold(c, got, label):
    val, mag = reference(c, got["y"])
    if c["x"].shape[0]:
        live = mag["y"] > 0
        assert (got["y"][live] > 0).any() and (got["y"][live] < 0).any(), "dy must straddle y = 0"
    bad = []
    for name, g in got.items():
        err = np.abs(g.astype(np.float64) - val[name])
        units = float((err / np.where(mag[name] > 0, mag[name], 1.0)).max()) if err.size else 0.0
        print("%s %-6s worst error %.2e of the sum of absolute terms" % (label, name, units))
        if not (err <= BAR * mag[name]).all():
            bad.append((name, units, int((err > BAR * mag[name]).sum())))
    assert not bad, bad
    return val, mag


def exact_zeros(c, got):
    """Rows without a group of y and dx, and an empty group's rows of dalpha and dbeta, are exact zeros."""
    if c["group"] is None:
        return
    bare = (c["group"] < 0) | (c["group"] >= c["G"])
    assert not got["y"][bare].any() and ("dx" not in got or not got["dx"][bare].any())
    for g in range(c["G"]):
        if not (c["group"] == g).any():
            assert ("dalpha" not in got or not got["dalpha"][g].any()) and ("dbeta" not in got or not got["dbeta"][g].any()), g


def same_bytes(a, b):
    """The tensors of a, bit for bit those of b (which may hold more)."""
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


# ---- head_out ---------------------------------------------------------------------------------------------------------
HEAD_FACTORS = {"xyz": 0.75, "rgb": 2.0, "scale": 0.5, "opacity": 0.6}


def head_reference(kind, f, w, b, factor):
    """(v, want, bar) of head_out in float64: the linear layer's value, the transform of it, and the bar per element --
    1e-5 * (sum_i |f_i W_ci| + |b_c|) * |transform'| plus one float32 unit of the result.  The clamp of `scale` has slope
    `factor` inside and 0 outside; a value within the bar of the clamp's corner may sit on either side of it, so the slope
    there is `factor` (the transform's Lipschitz constant).  b: the bias, or None."""
    b = np.zeros(w.shape[0], np.float32) if b is None else b
    v = f.astype(np.float64) @ w.astype(np.float64).T + b
    mag = np.abs(f).astype(np.float64) @ np.abs(w).astype(np.float64).T + np.abs(b)
    s = 1.0 / (1.0 + np.exp(-v))
    if kind == "scale":
        want, slope = 1.0 + np.clip(v, -1, 1) * factor, np.where(np.abs(v) <= 1 + BAR * mag, factor, 0.0)
    elif kind == "opacity":
        want, slope = s * factor + (1 - factor), s * (1 - s) * factor
    else:
        want, slope = (s - 0.5) * factor, s * (1 - s) * factor
    return v, want, BAR * mag * slope + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
