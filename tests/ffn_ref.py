"""What the GPU tests of the feed-forward operator (gcm_ffn_*) share: seeded inputs, the torch
formulation that serves as float64 target on the CPU and as float32 yardstick on the GPU, the operator, one forward +
backward of either, and the bar.

The bar.  Per tensor (y, dx and the six parameter gradients) the figure max|got - x64| / max|x64|, worst over the cases of
one (C, Hd), is at most 4 x the yardstick's same figure -- the project's factor for another summation order
(tests/test_attr_head_gpu.py) -- and the bar is never held below 2^-23, two float32 roundings of the largest element."""
import torch
import torch.nn.functional as F

TENSORS = ("y", "dx", "dln_w", "dln_b", "dw1", "db1", "dw2", "db2")
PARAMS = ("ln_w", "ln_b", "w1", "b1", "w2", "b2")
LEAVES = ("x",) + PARAMS                                # the seven differentiable inputs
EPS = 1e-5
FACTOR, FLOOR = 4.0, 2.0 ** -23


def make_inputs(N, C, Hd, seed):
    """Seeded normals; gamma = 1 + 0.5 n, small beta / b1 / b2, weights scaled by 1 / sqrt(fan-in), dy normal."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {"x": n(N, C), "ln_w": 1 + 0.5 * n(C), "ln_b": 0.1 * n(C), "w1": n(Hd, C) / C ** 0.5, "b1": 0.1 * n(Hd),
            "w2": n(C, Hd) / Hd ** 0.5, "b2": 0.1 * n(C), "dy": n(N, C)}


def torch_ops(t, s):
    xn = F.layer_norm(t["x"], (t["x"].shape[1],), t["ln_w"], t["ln_b"], EPS)
    h = F.linear(F.gelu(F.linear(xn, t["w1"], t["b1"])), t["w2"], t["b2"])
    return t["x"] + (h if s is None else s[:, None] * h)


def fused(t, s):
    from gaussiancity_amd.ffn import layernorm_mlp_residual
    return layernorm_mlp_residual(t["x"], t["ln_w"], t["ln_b"], EPS, t["w1"], t["b1"], t["w2"], t["b2"], s)


def run(fn, inp, device, dtype, s=None, stride=None, need=LEAVES):
    """y and the seven gradients of fn on the device in dtype, one forward and one backward.  stride: x and dy as views
    of rows that far apart.  need: the leaves (of LEAVES) that require a gradient, not empty; the gradient of any other
    leaf comes back as None, which is what its .grad is."""
    assert need and set(need) <= set(LEAVES), need
    t = {k: inp[k].detach().clone().to(device=device, dtype=dtype).requires_grad_(k in need) for k in LEAVES}
    dy = inp["dy"].to(device=device, dtype=dtype)
    if s is not None:
        s = s.to(device=device, dtype=dtype)
    leaf = t["x"]
    if stride is not None:
        N, C = leaf.shape
        wide = torch.zeros((N, stride), device=device, dtype=dtype)
        wide[:, :C] = leaf.detach()
        leaf = wide.requires_grad_("x" in need)
        t["x"] = leaf[:, :C]
        wide_dy = torch.full((N, stride), 7.0, device=device, dtype=dtype)
        wide_dy[:, :C] = dy
        dy = wide_dy[:, :C]
    y = fn(t, s)
    y.backward(dy)
    out = {"y": y.detach(), "dx": leaf.grad if stride is None or leaf.grad is None else leaf.grad[:, :inp["x"].shape[1]]}
    out.update({"d" + k: t[k].grad for k in PARAMS})
    return {k: None if v is None else v.detach().cpu() for k, v in out.items()}


def figures(got, want):
    """max|got - x64| / max|x64| per tensor."""
    return {k: float((got[k].double() - want[k]).abs().max() / want[k].abs().max()) for k in TENSORS}


def check_bar(label, cases, dev):
    """cases: (inputs, row_scale) pairs that share one (C, Hd): the worst figure of the operator over the cases against
    the worst of the yardstick, per tensor."""
    worst_got, worst_yard = dict.fromkeys(TENSORS, 0.0), dict.fromkeys(TENSORS, 0.0)
    for inp, s in cases:
        want = run(torch_ops, inp, "cpu", torch.float64, s)
        got, yard = figures(run(fused, inp, dev, torch.float32, s), want), figures(run(torch_ops, inp, dev, torch.float32, s), want)
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


def same_bits(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in TENSORS)
