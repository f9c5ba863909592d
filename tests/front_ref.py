"""What the tests of the Block-front operator (gcm_front_*) share: seeded inputs, the torch
formulation that serves as float64 target on the CPU and as float32 yardstick on the GPU, the operator, one forward +
backward of either, and the bar.

The formulation:  t = s Wc^T + bc;  feat = x + LN_c(t);  qkv = LN_1(feat) Wq^T + bq;  the loss is
(feat * wf).sum() + (qkv * wqkv).sum() with seeded normal weights, i.e. the backward is fed dfeat = wf and dqkv = wqkv.

The bar (section 18's, unchanged).  Per tensor (feat, qkv, dx, ds and the eight parameter gradients) the figure
max|got - x64| / max|x64|, worst over the cases of one (C, O), is at most 4 x the yardstick's same figure -- the project's
factor for another summation order -- and the bar is never held below 2^-23, two float32 roundings of the largest element."""
import torch
import torch.nn.functional as F

PARAMS = ("wc", "bc", "gc", "bec", "g1", "be1", "wq", "bq")
LEAVES = ("x", "s") + PARAMS                             # the ten differentiable inputs
TENSORS = ("feat", "qkv", "dx", "ds") + tuple("d" + k for k in PARAMS)
EPS_C, EPS_1 = 1e-5, 1e-6                                # two different eps: a swap shows
FACTOR, FLOOR = 4.0, 2.0 ** -23


def make_inputs(N, C, O, seed):
    """Seeded normals; gamma = 1 + 0.5 n, small biases, weights scaled by 1 / sqrt(fan-in), the loss weights normal."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {"x": n(N, C), "s": n(N, C), "wc": n(C, C) / C ** 0.5, "bc": 0.1 * n(C), "gc": 1 + 0.5 * n(C), "bec": 0.1 * n(C),
            "g1": 1 + 0.5 * n(C), "be1": 0.1 * n(C), "wq": n(O, C) / C ** 0.5, "bq": 0.1 * n(O), "dfeat": n(N, C),
            "dqkv": n(N, O)}


def special_rows(inp):
    """A constant bias with a zero row of s (t exactly constant: variance 0, rstd = 1 / sqrt(eps)), a row of s scaled by
    1e6, a row of x scaled by 1e3 beside one scaled by 1e-3.  N >= 9.  (No row of s scaled DOWN under the constant bias:
    a nearly constant t cancels in float32 itself, which would test the inputs and not the kernel.)"""
    x, s = inp["x"].clone(), inp["s"].clone()
    assert x.shape[0] >= 9
    s[3] = 0.0
    s[5] *= 1e6
    x[6] *= 1e3
    x[7] *= 1e-3
    return dict(inp, x=x, s=s, bc=torch.full_like(inp["bc"], 0.25))


def torch_ops(t):
    C = t["x"].shape[1]
    u = F.layer_norm(F.linear(t["s"], t["wc"], t["bc"]), (C,), t["gc"], t["bec"], EPS_C)
    feat = t["x"] + u
    return feat, F.linear(F.layer_norm(feat, (C,), t["g1"], t["be1"], EPS_1), t["wq"], t["bq"])


def fused(t):
    from gaussiancity_amd.front import conv_tail_norm_qkv
    return conv_tail_norm_qkv(t["x"], t["s"], t["wc"], t["bc"], t["gc"], t["bec"], EPS_C, t["g1"], t["be1"], EPS_1, t["wq"],
                              t["bq"])


def _wide(value, extra, fill, need):
    """value [N, W] as a view of rows W + extra apart; the leaf is the wide tensor."""
    N, W = value.shape
    wide = torch.full((N, W + extra), fill, device=value.device, dtype=value.dtype)
    wide[:, :W] = value
    wide.requires_grad_(need)
    return wide, wide[:, :W]


def run(fn, inp, device, dtype, strided=False, need=LEAVES):
    """feat, qkv and the ten gradients of fn on the device in dtype, one forward and one backward.  strided: x, s, dfeat
    and dqkv as views of rows 4 elements further apart.  need: the leaves (of LEAVES) that require a gradient, not empty;
    the gradient of any other leaf comes back as None, which is what its .grad is."""
    assert need and set(need) <= set(LEAVES), need
    t = {k: inp[k].detach().clone().to(device=device, dtype=dtype).requires_grad_(k in need) for k in LEAVES}
    dfeat, dqkv = (inp[k].to(device=device, dtype=dtype) for k in ("dfeat", "dqkv"))
    leaf = {"x": t["x"], "s": t["s"]}
    if strided:
        for k in ("x", "s"):
            leaf[k], t[k] = _wide(t[k].detach(), 4, 0.0, k in need)
        dfeat, dqkv = _wide(dfeat, 4, 7.0, False)[1], _wide(dqkv, 4, 7.0, False)[1]
    feat, qkv = fn(t)
    torch.autograd.backward([feat, qkv], [dfeat, dqkv])
    C = inp["x"].shape[1]
    out = {"feat": feat.detach(), "qkv": qkv.detach()}
    out.update({"d" + k: None if leaf[k].grad is None else leaf[k].grad[:, :C] for k in ("x", "s")})
    out.update({"d" + k: t[k].grad for k in PARAMS})
    return {k: None if v is None else v.detach().cpu() for k, v in out.items()}


def figures(got, want):
    """max|got - x64| / max|x64| per tensor."""
    return {k: float((got[k].double() - want[k]).abs().max() / want[k].abs().max()) for k in TENSORS}


def check_bar(label, cases, dev, strided=False):
    """cases: inputs that share one (C, O): the worst figure of the operator over the cases against the worst of the
    yardstick, per tensor.  Every figure is printed before anything is asserted."""
    worst_got, worst_yard = dict.fromkeys(TENSORS, 0.0), dict.fromkeys(TENSORS, 0.0)
    for inp in cases:
        want = run(torch_ops, inp, "cpu", torch.float64)
        got = figures(run(fused, inp, dev, torch.float32, strided), want)
        yard = figures(run(torch_ops, inp, dev, torch.float32), want)
        for k in TENSORS:
            worst_got[k], worst_yard[k] = max(worst_got[k], got[k]), max(worst_yard[k], yard[k])
    failed = []
    for k in TENSORS:
        bar = max(FACTOR * worst_yard[k], FLOOR)
        print("%s %-5s operator %.3e  torch float32 %.3e  ratio %.2f  bar %.3e" % (
            label, k, worst_got[k], worst_yard[k], worst_got[k] / max(worst_yard[k], 1e-30), bar))
        if not worst_got[k] <= bar:
            failed.append((k, worst_got[k], bar))
    assert not failed, failed


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b, names=TENSORS):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in names)
