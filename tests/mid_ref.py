"""What the tests of the Block-middle operators (gcm_mid_*) share: seeded index pairs and inputs, the
torch formulation that serves as float64 target on the CPU and as float32 yardstick on the GPU, the operators, one forward +
backward of either, and the bar.

The formulation:  packed = qkv[order];  p = a[inverse] Wp^T + bp;  y = x + p, or x + p * r[:, None];  the loss is
(packed * wg).sum() + (y * wy).sum() with seeded normal weights, i.e. the backwards are fed dpacked = wg and dy = wy.

The bar (tests/front_ref.py's, unchanged).  Per tensor (y, da, dwp, dbp) the figure max|got - x64| / max|x64|, worst over
the cases of one C, is at most 4 x the yardstick's same figure -- the project's factor for another summation order -- and
the bar is never held below 2^-23.  packed, dqkv and dx are held to torch's bits, not to a bar."""
import torch
import torch.nn.functional as F

from front_ref import FACTOR, FLOOR, bits  # noqa: F401

LEAVES = ("qkv", "a", "x", "wp", "bp")                   # the differentiable inputs
TENSORS = ("y", "da", "dwp", "dbp")                      # held to the bar
EXACT = ("packed", "dqkv", "dx")                         # held to torch's bits
KEEP = 0.7


def make_indices(N, D, seed, identity=False):
    """(order [N + D], inverse [N], extra [N]): order is a permutation of the rows (the identity on request) with D
    duplicates of distinct rows at interleaved slots, inverse[n] the row's own slot, extra[n] its duplicate slot or -1."""
    assert 0 <= D <= N
    g = torch.Generator().manual_seed(seed)
    perm = torch.arange(N) if identity else torch.randperm(N, generator=g)
    dup_rows = torch.randperm(N, generator=g)[:D]
    T = N + D
    dup_slots = torch.randperm(T, generator=g)[:D].sort().values
    is_dup = torch.zeros(T, dtype=torch.bool)
    is_dup[dup_slots] = True
    order = torch.empty(T, dtype=torch.int64)
    order[~is_dup], order[is_dup] = perm, dup_rows
    inverse = torch.empty(N, dtype=torch.int64)
    inverse[perm] = torch.nonzero(~is_dup)[:, 0]
    extra = torch.full((N,), -1, dtype=torch.int32)
    extra[dup_rows] = dup_slots.int()
    assert torch.equal(order[inverse], torch.arange(N))
    return order, inverse, extra


def extra_numpy(order, inverse):
    """slot_plan in numpy: the slots that are not their row's own, by row."""
    import numpy as np
    o, i = order.numpy(), inverse.numpy()
    extra = np.full(len(i), -1, np.int32)
    dup = np.nonzero(i[o] != np.arange(len(o)))[0]
    extra[o[dup]] = dup
    return extra


def make_inputs(N, D, C, seed, W=None, scale=True, identity=False):
    """Seeded normals; the weight scaled by 1 / sqrt(fan-in), a small bias, the loss weights normal.  W: the width of the
    gathered rows (3 C by default).  scale: a row scale of zeros and 1 / KEEP that holds both when N > 1."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    order, inverse, extra = make_indices(N, D, seed + 1, identity)
    W = 3 * C if W is None else W
    inp = {"qkv": n(N, W), "a": n(N + D, C), "x": n(N, C), "wp": n(C, C) / C ** 0.5, "bp": 0.1 * n(C), "wg": n(N + D, W),
           "wy": n(N, C), "order": order, "inverse": inverse, "extra": extra, "r": None}
    if scale:
        r = (torch.rand(N, generator=g) < KEEP).float() / KEEP
        r[0] = 1 / KEEP
        if N > 1:
            r[N // 2] = 0.0
        inp["r"] = r
    return inp


def torch_ops(t, order, inverse, extra, r):
    p = F.linear(t["a"][inverse], t["wp"], t["bp"])
    if r is not None:
        p = p * r[:, None]
    return t["qkv"][order], t["x"] + p


def fused(t, order, inverse, extra, r):
    from gaussiancity_amd import mid
    return mid.gather_rows(t["qkv"], order, inverse, extra), mid.proj_residual(t["a"], inverse, extra, t["x"], t["wp"], t["bp"], r)


def _wide(value, extra_cols, fill, need):
    """value [N, W] as a view of rows W + extra_cols apart; the leaf is the wide tensor."""
    N, W = value.shape
    wide = torch.full((N, W + extra_cols), fill, device=value.device, dtype=value.dtype)
    wide[:, :W] = value
    wide.requires_grad_(need)
    return wide, wide[:, :W]


def run(fn, inp, device, dtype, strided=False, need=LEAVES, retain=False):
    """packed, y and the five gradients of fn on the device in dtype, one forward and one backward.  strided: qkv, a, x,
    dpacked and dy as views of rows 4 elements further apart.  Returns (results on the CPU, the live (outputs, leaves,
    gradients fed) for a test that runs the backward again)."""
    t = {k: inp[k].detach().clone().to(device=device, dtype=dtype).requires_grad_(k in need) for k in LEAVES}
    wg, wy = (inp[k].to(device=device, dtype=dtype) for k in ("wg", "wy"))
    order, inverse, extra = (inp[k].to(device) for k in ("order", "inverse", "extra"))
    r = None if inp["r"] is None else inp["r"].to(device=device, dtype=dtype)
    leaf = dict(t)
    if strided:
        for k in ("qkv", "a", "x"):
            leaf[k], t[k] = _wide(t[k].detach(), 4, 0.0, k in need)
        wg, wy = _wide(wg, 4, 7.0, False)[1], _wide(wy, 4, 7.0, False)[1]
    packed, y = fn(t, order, inverse, extra, r)
    live = [(o, w) for o, w in ((packed, wg), (y, wy)) if o.requires_grad]   # `need` may leave one output without a graph
    torch.autograd.backward([o for o, _ in live], [w for _, w in live], retain_graph=retain)
    width = {"qkv": inp["qkv"].shape[1], "a": inp["a"].shape[1], "x": inp["x"].shape[1]}
    out = {"packed": packed.detach(), "y": y.detach()}
    out.update({"d" + k: None if leaf[k].grad is None else leaf[k].grad[:, :width[k]] for k in ("qkv", "a", "x")})
    out.update({"d" + k: leaf[k].grad for k in ("wp", "bp")})
    return {k: None if v is None else v.detach().cpu().clone() for k, v in out.items()}, ((packed, y), leaf, (wg, wy))


def figures(got, want):
    """max|got - x64| / max|x64| per tensor of TENSORS."""
    return {k: float((got[k].double() - want[k]).abs().max() / want[k].abs().max()) for k in TENSORS}


def check_bar(label, cases, dev, strided=False):
    """cases: inputs that share one C: the worst figure of the operator over the cases against the worst of the yardstick,
    per tensor; packed, dqkv and dx against the yardstick's bits and the duplicate slots' rows of da against zero, per case.
    Every figure is printed before anything is asserted."""
    worst_got, worst_yard = dict.fromkeys(TENSORS, 0.0), dict.fromkeys(TENSORS, 0.0)
    inexact = []
    for inp in cases:
        want = run(torch_ops, inp, "cpu", torch.float64)[0]
        res = run(fused, inp, dev, torch.float32, strided)[0]
        yres = run(torch_ops, inp, dev, torch.float32)[0]
        got, yard = figures(res, want), figures(yres, want)
        for k in TENSORS:
            worst_got[k], worst_yard[k] = max(worst_got[k], got[k]), max(worst_yard[k], yard[k])
        shape = (inp["x"].shape[0], inp["a"].shape[0] - inp["x"].shape[0])
        inexact += [(shape, k) for k in EXACT if not torch.equal(res[k], yres[k])]
        if not torch.equal(res["dx"], inp["wy"]):
            inexact.append((shape, "dx is not the incoming gradient"))
        dup = inp["extra"][inp["extra"] >= 0].long()
        if not torch.equal(bits(res["da"][dup]), torch.zeros_like(bits(res["da"][dup]))):
            inexact.append((shape, "da is not +0 at the duplicate slots"))
    failed = []
    for k in TENSORS:
        bar = max(FACTOR * worst_yard[k], FLOOR)
        print("%s %-5s operator %.3e  torch float32 %.3e  ratio %.2f  bar %.3e" % (
            label, k, worst_got[k], worst_yard[k], worst_got[k] / max(worst_yard[k], 1e-30), bar))
        if not worst_got[k] <= bar:
            failed.append((k, worst_got[k], bar))
    assert not failed and not inexact, (failed, inexact)


def same_bits(a, b, names=TENSORS + EXACT):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in names)
