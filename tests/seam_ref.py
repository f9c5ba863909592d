"""What the tests of the stage-seam operator (gcm_seam_*) share: seeded inputs, the torch formulation
that serves as float64 target on the CPU and as float32 yardstick on the GPU, the operator, one forward + backward of
either, and the bar.

The formulation:  z = F.linear(x, w, b) (or x itself without a product);  u = F.batch_norm(z, running_mean, running_var, g,
h, training, momentum, eps);  y = F.gelu(u) (or u);  the loss is (y * dy).sum() with seeded normal dy.  F.batch_norm updates
the two running buffers in training mode; the counter is BatchNorm1d's own line and is added here.

The bar (tests/mid_ref.py's, unchanged).  Per tensor the figure max|got - x64| / max|x64|, worst over the cases of one
(I, O), is at most 4 x the yardstick's same figure -- the project's factor for another summation order -- and the bar is
never held below 2^-23.  Two tensors need another scale: db in front of batch statistics is mathematically 0 (the norm
removes what a bias adds) and is measured against dw's maximum, as tests/test_point_pool_gpu.py measures its bias gradient;
the running statistics are measured against their own maximum, which is what the figure does."""
import torch
import torch.nn.functional as F

from front_ref import FACTOR, FLOOR

LEAVES = ("x", "w", "b", "g", "h")
GRADS = ("dx", "dw", "db", "dg", "dh")
TENSORS = ("y",) + GRADS + ("running_mean", "running_var")
EPS, MOMENTUM = 1e-3, 0.01   # PTv3's BatchNorm1d
FAR = 1                      # the column of z whose mean is 100 standard deviations


def bits(t):
    return t.contiguous().view(torch.int32)


def make_inputs(N, I, O, seed, product=True, exact=False, drift=0.0):
    """Seeded normals: w scaled by 1 / sqrt(fan-in), small biases, g = 1 + 0.5 n, non-trivial running statistics and a
    counter at 7.  Column FAR of z gets a mean of 100 standard deviations (through b, or through x without a product): the
    case that a sum z^2 - (sum z)^2 / N formulation loses.  product=False: x is [N, O].
    drift: a ramp linspace(0, drift, N) over the rows, as the features of a serialised point cloud move along its curve:
    the tiles' means then differ and the correction term of the variance merge carries most of the variance.  With the
    product it is added to column 0 of x (every column of z drifts through w[:, 0]), without it to column 2 of x."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if not product:
        I = O
    inp = {"x": n(N, I), "w": n(O, I) / I ** 0.5, "b": 0.1 * n(O), "g": 1 + 0.5 * n(O), "h": 0.1 * n(O), "dy": n(N, O),
           "running_mean": 0.3 * n(O), "running_var": 0.5 + torch.rand(O, generator=g),
           "tracked": torch.tensor(7, dtype=torch.int64)}
    if product:
        inp["b"][FAR] = 100.0
    else:
        inp["w"] = inp["b"] = None
        inp["x"][:, FAR] += 100.0
    if drift:
        inp["x"][:, 0 if product else 2] += torch.linspace(0, drift, N)
    return inp


def torch_ops(t, buf, training, act, momentum=MOMENTUM):
    z = t["x"] if t["w"] is None else F.linear(t["x"], t["w"], t["b"])
    u = F.batch_norm(z, buf["running_mean"], buf["running_var"], t["g"], t["h"], training, momentum, EPS)
    if training:
        buf["tracked"] += 1
    return F.gelu(u) if act else u


def fused(t, buf, training, act, momentum=MOMENTUM):
    from gaussiancity_amd import seam
    return seam.linear_bn_gelu(t["x"], t["w"], t["b"], t["g"], t["h"], buf["running_mean"], buf["running_var"], buf["tracked"],
                               training=training, momentum=momentum, eps=EPS, act=act)


def _wide(value, extra_cols, fill, need):
    """value [N, W] as a view of rows W + extra_cols apart; the leaf is the wide tensor."""
    N, W = value.shape
    wide = torch.full((N, W + extra_cols), fill, device=value.device, dtype=value.dtype)
    wide[:, :W] = value
    wide.requires_grad_(need)
    return wide, wide[:, :W]


def run(fn, inp, device, dtype, training, act, strided=False, need=LEAVES, retain=False, grad=True, momentum=MOMENTUM):
    """y, the gradients of `need` and the three buffers after one forward (+ backward) of fn on the device in dtype.
    strided: x and dy as views of rows 4 elements further apart.  momentum = 1.0: the buffers afterwards are the batch mean
    and the unbiased batch variance.  Returns (results on the CPU, live (y, leaves, dy, buf))."""
    t = {k: None if inp[k] is None else inp[k].detach().clone().to(device=device, dtype=dtype).requires_grad_(grad and k in need)
         for k in LEAVES}
    buf = {k: inp[k].clone().to(device=device, dtype=dtype) for k in ("running_mean", "running_var")}
    buf["tracked"] = inp["tracked"].clone().to(device)
    dy = inp["dy"].to(device=device, dtype=dtype)
    leaf = dict(t)
    if strided:
        leaf["x"], t["x"] = _wide(t["x"].detach(), 4, 0.0, grad and "x" in need)
        dy = _wide(dy, 4, 7.0, False)[1]
    if grad:
        y = fn(t, buf, training, act, momentum)
        if y.requires_grad:
            y.backward(dy, retain_graph=retain)
    else:
        with torch.no_grad():
            y = fn(t, buf, training, act, momentum)
    out = {"y": y.detach()}
    for k in LEAVES:
        gr = None if leaf[k] is None else leaf[k].grad
        out["d" + k] = gr[:, :inp["x"].shape[1]] if (k == "x" and gr is not None) else gr
    out.update(buf)
    return {k: None if v is None else v.detach().cpu().clone() for k, v in out.items()}, (y, leaf, dy, buf)


def figures(got, want, training):
    """max|got - x64| / max|x64| per tensor that exists; db under batch statistics against dw's maximum."""
    fig = {}
    for k in TENSORS:
        if want.get(k) is None:
            continue
        scale = want["dw"] if (k == "db" and training) else want[k]
        fig[k] = float((got[k].double() - want[k]).abs().max() / scale.abs().max())
    return fig


def check_bar(label, cases, dev, strided=False, momentum=MOMENTUM):
    """cases: (inputs, training, act) that share one (I, O): the worst figure of the operator over the cases against the
    worst of the yardstick, per tensor; the counter exact.  Every figure is printed before anything is asserted."""
    worst_got, worst_yard = dict.fromkeys(TENSORS, 0.0), dict.fromkeys(TENSORS, 0.0)
    wrong = []
    for inp, training, act in cases:
        want = run(torch_ops, inp, "cpu", torch.float64, training, act, momentum=momentum)[0]
        res = run(fused, inp, dev, torch.float32, training, act, strided, momentum=momentum)[0]
        yres = run(torch_ops, inp, dev, torch.float32, training, act, momentum=momentum)[0]
        got, yard = figures(res, want, training), figures(yres, want, training)
        for k in got:
            worst_got[k], worst_yard[k] = max(worst_got[k], got[k]), max(worst_yard[k], yard[k])
        if int(res["tracked"]) != int(want["tracked"]):
            wrong.append((tuple(inp["x"].shape), training, "counter", int(res["tracked"])))
        if not training and not (torch.equal(res["running_mean"], inp["running_mean"])
                                 and torch.equal(res["running_var"], inp["running_var"])):
            wrong.append((tuple(inp["x"].shape), "eval mode touched the running buffers"))
    failed = []
    for k in TENSORS:
        bar = max(FACTOR * worst_yard[k], FLOOR)
        print("%s %-12s operator %.3e  torch float32 %.3e  ratio %.2f  bar %.3e" % (
            label, k, worst_got[k], worst_yard[k], worst_got[k] / max(worst_yard[k], 1e-30), bar))
        if not worst_got[k] <= bar:
            failed.append((k, worst_got[k], bar))
    assert not failed and not wrong, (failed, wrong)


def same_bits(a, b, names=TENSORS):
    return all((a[k] is None and b[k] is None) or torch.equal(bits(a[k]), bits(b[k])) for k in names)
