"""Operand views for the public operators: every tensor operand of an operator, handed over as a legal torch view of the
same values, must give the bits that its dense, allocator-aligned twin gives -- forward and backward.

  build(kind, t, dim=None) -> Built    one view of t's values (KINDS), with the buffer under it and the property the kind
                                       is there for asserted
  Operand / Op / REGISTRY              the table: per operator a seeded case, a function that runs it, and per tensor
                                       operand the view kinds that apply
  sweep(op, device) -> int             runs the baseline and every registered (operand, kind) of op, asserts, counts
  PUBLIC                               the operators the sweep answers for, for the host-side completeness check

An operand is either an input of the operator (a key of the case that op.run reads) or an incoming gradient (role
"grad"): the gradient of one output, fed through backward() and checked with a hook to reach the operator as that view.
"""
import importlib

import torch

FILL = 7
KINDS = ("offset", "ragged_rows", "transposed", "expanded")


# ---- the views -------------------------------------------------------------------------------------------------------------
class Built:
    """view: the operand; base: the buffer under it (None: the view owns its memory); take(b): the view's region of a
    tensor shaped like base; filler: True when base holds FILL outside the region."""
    __slots__ = ("kind", "view", "base", "take", "filler")

    def __init__(self, kind, base, take, filler):
        self.kind, self.base, self.take, self.filler = kind, base, take, filler
        self.view = take(base)

    def outside(self, like=None):
        """The elements of `like` (base by default) that the view does not cover, as a 1-D tensor."""
        covered = torch.zeros(self.base.shape, dtype=torch.bool, device=self.base.device)
        self.take(covered).fill_(True)
        return (self.base if like is None else like)[~covered]


def _is_fill(x):
    """Every element of x is the filler, in x's dtype (True for a boolean buffer)."""
    return (x == torch.tensor(FILL).to(x.dtype).to(x.device)).all()


def _offset(t, dim):
    n = t.numel()
    base = torch.full((n + 2,), FILL, dtype=t.dtype, device=t.device)
    base[1:n + 1] = t.reshape(-1)
    b = Built("offset", base, lambda buf: buf[1:n + 1].view(t.shape), True)
    assert base.data_ptr() % 16 == 0, "the buffer under an offset view starts 16-byte aligned"
    assert b.view.is_contiguous() and b.view.storage_offset() == 1 and b.view.data_ptr() % 16 != 0
    assert t.element_size() != 2 or b.view.data_ptr() % 4 != 0
    return b


def _ragged_rows(t, dim):
    assert t.dim() >= 2, "ragged_rows needs rows"
    w = t.shape[-1]
    pad = 1 if (w + 1) % 4 else 2  # the row stride must be no multiple of 4 elements
    base = torch.full(tuple(t.shape[:-1]) + (w + pad,), FILL, dtype=t.dtype, device=t.device)
    base[..., 1:1 + w] = t
    b = Built("ragged_rows", base, lambda buf: buf[..., 1:1 + w], True)
    assert b.view.stride(-1) == 1 and b.view.stride(-2) == w + pad and b.view.stride(-2) % 4 != 0
    assert b.view.storage_offset() == 1 and (t.numel() <= w or not b.view.is_contiguous())  # one row alone is dense
    return b


def _transposed(t, dim):
    assert t.dim() == 2, "transposed is for matrices"
    base = t.t().contiguous()
    b = Built("transposed", base, lambda buf: buf.t(), False)
    want = (1, t.shape[0])  # column-major; the stride of a dimension of one element says nothing
    assert all(s == e for s, e, n in zip(b.view.stride(), want, t.shape) if n > 1)
    assert min(t.shape) == 1 or not b.view.is_contiguous()
    return b


def _expanded(t, dim):
    """The values of t's first slice along dim (every dimension when dim is None), with stride 0 there."""
    dims = range(t.dim()) if dim is None else (dim,)
    first = t
    for d in dims:
        first = first.narrow(d, 0, 1)
    base = first.clone()
    b = Built("expanded", base, lambda buf: buf.expand(t.shape), False)
    assert all(b.view.stride(d) == 0 for d in dims if t.shape[d] > 1)
    return b


_BUILDERS = {"offset": _offset, "ragged_rows": _ragged_rows, "transposed": _transposed, "expanded": _expanded}


def build(kind, t, dim=None):
    b = _BUILDERS[kind](t, dim)
    twin = t if kind != "expanded" else b.view.contiguous()
    assert b.view.shape == t.shape and b.view.dtype == t.dtype and bits_equal(b.view, twin), kind
    if b.filler:
        assert bool(_is_fill(b.outside())), kind
    return b


def bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


# ---- the table -------------------------------------------------------------------------------------------------------------
class Refuses:
    """A view the operator documents as refused: the call must raise `error` with `message` in it."""

    def __init__(self, kind, error, message, why):
        self.kind, self.error, self.message, self.why = kind, error, message, why


class Operand:
    """kinds: names of KINDS or Refuses entries.  diff: a float input that gets a gradient.  role: "in", "grad" (the
    incoming gradient of output `of`) or "inplace" (the operator updates it; its new values are a result).  dim: the
    dimension "expanded" broadcasts (None: all).  param: the parameter of the public signature it is (part of)."""

    def __init__(self, kinds, diff=False, role="in", of=None, dim=None, param=None):
        self.kinds, self.diff, self.role, self.of, self.dim, self.param = tuple(kinds), diff, role, of, dim, param


class Op:
    """id; lib: the HIP library under it; target: "module:attribute" of the public operator; make(gen) -> {name: CPU
    tensor}; run(t) -> {output name: tensor} from the operands on the device; operands {name: Operand}; skipped
    {parameter: reason} for the parameters of the signature that hold no tensor operand of the sweep; setup(device) ->
    teardown callable, around every run; bars {result name: bar(case) -> (exact value, bound), float64 CPU tensors} for
    the results documented as not bit-reproducible: each run's result is held to |got - exact| <= bound, the module's own
    bar, and every other result to the twin's bits."""

    def __init__(self, id, lib, target, make, run, operands, skipped=None, setup=None, parameters=None, bars=None):
        self.id, self.lib, self.target, self.make, self.run = id, lib, target, make, run
        self.operands, self.skipped, self.setup, self._parameters = operands, dict(skipped or {}), setup, parameters
        self.bars = dict(bars or {})

    def parameters(self):
        """The names that can hold a tensor operand: the public function's parameters; for a module class, whose
        signature is its constructor's, the names given with the entry (its forward's tensors and its parameters)."""
        if self._parameters is not None:
            return tuple(self._parameters)
        import inspect
        return tuple(inspect.signature(self.public()).parameters)

    def covered(self, parameter):
        """The operands that are (part of) `parameter`: named by Operand.param, else by the name up to the first dot."""
        return {n: o for n, o in self.operands.items() if o.role != "grad" and (o.param or n.split(".")[0]) == parameter}

    def pairs(self):
        return [(name, k) for name, o in self.operands.items() for k in o.kinds]

    def public(self):
        mod, attr = self.target.split(":")
        return getattr(importlib.import_module(mod), attr)


def _kind_name(k):
    return k.kind if isinstance(k, Refuses) else k


def _execute(op, case, dev, sub=None):
    """One forward + backward of op.  sub = (operand name, kind or Refuses): that operand goes in as the view.  Returns
    {result name: CPU tensor or None}; for sub also checks what only a view can show."""
    t, leaves, built = {}, {}, None
    for name, o in op.operands.items():
        v = case[name]
        if v is None:
            t[name] = None
            continue
        v = v.clone().to(dev)
        if sub is not None and sub[0] == name:
            built = build(_kind_name(sub[1]), v, o.dim)
            if o.diff and built.kind == "expanded":  # the leaf is the broadcast tensor itself, as an expanded gradient is
                v = leaves[name] = built.view.detach().requires_grad_(True)
            elif o.diff:
                built.base.requires_grad_(True)
                leaves[name] = built.base
                v = built.take(built.base)
            else:
                v = built.view
        elif o.diff:
            v.requires_grad_(True)
            leaves[name] = v
        t[name] = v
    for name, v in case.items():
        if name not in op.operands:
            t[name] = v.to(dev) if isinstance(v, torch.Tensor) else v
    before = None if built is None or built.base is None else built.base.detach().clone()
    outs = op.run(t)
    res = {"out:" + k: v.detach() for k, v in outs.items()}
    grads = [(name, o) for name, o in op.operands.items() if o.role == "grad"]
    if grads:
        seen = []
        for name, o in grads:
            if sub is not None and sub[0] == name:
                outs[o.of].register_hook(lambda g: seen.append((g.data_ptr(), g.stride())))
        torch.autograd.backward([outs[o.of] for _, o in grads], [t[name] for name, _ in grads])
        if sub is not None and op.operands[sub[0]].role == "grad":
            g = t[sub[0]]
            assert seen == [(g.data_ptr(), g.stride())], "autograd handed the operator another gradient than the view"
        for name, leaf in leaves.items():
            g = leaf.grad
            if built is not None and sub[0] == name and g is not None and built.kind != "expanded":
                assert g.shape == built.base.shape
                if built.filler:
                    assert bool((built.outside(g) == 0).all()), "%s: gradient outside the viewed region" % name
                g = built.take(g)
            res["grad:" + name] = None if g is None else g.detach()
    for name, o in op.operands.items():
        if o.role == "inplace" and t[name] is not None:
            res["state:" + name] = t[name].detach()
    if built is not None and built.base is not None:
        now = built.base.detach()
        if built.filler:
            assert bool(_is_fill(built.outside(now))), "%s: the call wrote outside the view" % sub[0]
        if op.operands[sub[0]].role != "inplace":
            assert bits_equal(now, before), "%s: the call changed an operand it only reads" % sub[0]
    return {k: None if v is None else v.cpu() for k, v in res.items()}


def _twin_case(op, case, name):
    """The case whose `name` holds what the expanded view holds, materialised."""
    twin = dict(case)
    twin[name] = build("expanded", case[name], op.operands[name].dim).view.contiguous()
    return twin


def sweep(op, dev):
    """Baseline + every registered (operand, kind); returns the number of views run.  Collects every mismatch."""
    teardown = op.setup(dev) if op.setup else None
    try:
        case = op.make(torch.Generator().manual_seed(20))
        base = _execute(op, case, dev)
        assert base and all(v is not None for k, v in base.items() if k.startswith("out:")), op.id
        again = _execute(op, case, dev)
        assert set(op.bars) <= set(base), (op.id, sorted(base))
        assert sorted(base) == sorted(again) and all(bits_equal(base[k], again[k]) for k in base if k not in op.bars), \
            "%s: two dense runs differ" % op.id
        bad, ran = [], 0
        for name, o in op.operands.items():
            if o.role == "inplace":
                assert not bits_equal(base["state:" + name], case[name]), "%s: the case leaves %s as it was" % (op.id, name)
        for k, bar in op.bars.items():
            beyond = _beyond(base[k], bar(case))
            assert not beyond, "%s: the dense run's %s is beyond its bar at %d elements" % (op.id, k, beyond)
        for name, kind in op.pairs():
            ran += 1
            if case[name] is None:
                raise AssertionError("%s: the case has no %s" % (op.id, name))
            if isinstance(kind, Refuses):
                try:
                    _execute(op, case, dev, (name, kind))
                except kind.error as e:
                    if kind.message not in str(e):
                        bad.append("%s %s: refused with %r, not with %r" % (name, kind.kind, str(e), kind.message))
                else:
                    bad.append("%s %s: accepted, documented as refused (%s)" % (name, kind.kind, kind.why))
                continue
            used = case if kind != "expanded" else _twin_case(op, case, name)
            want = base if kind != "expanded" else _execute(op, used, dev)
            try:
                got = _execute(op, case, dev, (name, kind))
            except (RuntimeError, ValueError, TypeError, NotImplementedError, AssertionError) as e:
                if "hip" in str(e).lower():  # the device's error, not an argument check's: nothing more runs on it
                    raise
                bad.append("%s %s: %s: %s" % (name, kind, type(e).__name__, str(e)[:300]))
                continue
            for k in want:
                if k not in got:
                    bad.append("%s %s: no result %s" % (name, kind, k))
                elif k in op.bars:
                    beyond = _beyond(got[k], op.bars[k](used))
                    if beyond:
                        bad.append("%s %s: %s is beyond its bar at %d elements" % (name, kind, k, beyond))
                elif not bits_equal(got[k], want[k]):
                    bad.append("%s %s: %s differs from the dense twin's%s" % (name, kind, k, _worst(got[k], want[k])))
        assert not bad, "%s: %d of %d views fail\n  " % (op.id, len(bad), ran) + "\n  ".join(bad)
        return ran
    finally:
        if teardown:
            teardown()


def _beyond(got, bar):
    """The number of elements of got further from the bar's exact value than its bound."""
    exact, bound = bar
    return int(((got.double() - exact).abs() > bound).sum()) if got.shape == exact.shape else got.numel() + 1


def _worst(a, b):
    if a is None or b is None or a.shape != b.shape or not a.dtype.is_floating_point:
        return ""
    d = (a.double() - b.double()).abs()
    return " (max |diff| %.3g at %d of %d elements)" % (float(d.max()) if d.numel() else 0.0, int((d != 0).sum()), d.numel())


# ---- kinds by the operand's shape ----------------------------------------------------------------------------------------------
VEC = ("offset",)
VECX = ("offset", "expanded")
MAT = ("offset", "ragged_rows", "transposed")
GRAD = ("offset", "ragged_rows", "transposed", "expanded")
ND = ("offset", "ragged_rows")
NDG = ("offset", "ragged_rows", "expanded")


def _randn(gen, *shape, scale=1.0):
    return torch.randn(shape, generator=gen) * scale


def _grad_of(of, kinds=GRAD, **kw):
    return Operand(kinds, role="grad", of=of, **kw)


def _f(kinds=MAT, **kw):
    return Operand(kinds, diff=True, **kw)


# ---- libgcm ----------------------------------------------------------------------------------------------------------------
def _ffn(C, split):
    N, Hd = 65, 72 if C > 4 else 8

    def make(gen):
        return {"x": _randn(gen, N, C), "ln_weight": _randn(gen, C), "ln_bias": _randn(gen, C), "w1": _randn(gen, Hd, C, scale=C ** -0.5),
                "b1": _randn(gen, Hd), "w2": _randn(gen, C, Hd, scale=Hd ** -0.5), "b2": _randn(gen, C),
                "row_scale": (torch.rand(N, generator=gen) < 0.7).float() / 0.7, "dy": _randn(gen, N, C)}

    def run(t):
        from gaussiancity_amd import ffn
        return {"y": ffn.layernorm_mlp_residual(t["x"], t["ln_weight"], t["ln_bias"], 1e-5, t["w1"], t["b1"], t["w2"], t["b2"],
                                                t["row_scale"], split=split)}
    ops = {"x": _f(), "ln_weight": _f(VEC), "ln_bias": _f(VEC), "w1": _f(), "b1": _f(VECX), "w2": _f(), "b2": _f(VECX),
           "row_scale": Operand(VECX), "dy": _grad_of("y")}
    return Op("ffn.layernorm_mlp_residual[C=%d,split=%s]" % (C, split), "gcm", "gaussiancity_amd.ffn:layernorm_mlp_residual",
              make, run, ops, {"eps": "a number", "split": "a flag"})


def _front(C):
    N, O = 65, 3 * C if C > 4 else 8
    vecs = ("bc", "lnc_w", "lnc_b", "ln1_w", "ln1_b")

    def make(gen):
        c = {"x": _randn(gen, N, C), "s": _randn(gen, N, C), "wc": _randn(gen, C, C, scale=C ** -0.5),
             "wq": _randn(gen, O, C, scale=C ** -0.5), "bq": _randn(gen, O), "dfeat": _randn(gen, N, C), "dqkv": _randn(gen, N, O)}
        c.update({k: _randn(gen, C) for k in vecs})
        return c

    def run(t):
        from gaussiancity_amd import front
        feat, qkv = front.conv_tail_norm_qkv(t["x"], t["s"], t["wc"], t["bc"], t["lnc_w"], t["lnc_b"], 1e-5, t["ln1_w"], t["ln1_b"],
                                             1e-5, t["wq"], t["bq"])
        return {"feat": feat, "qkv": qkv}
    ops = {"x": _f(), "s": _f(), "wc": _f(), "wq": _f(), "bq": _f(VECX), "dfeat": _grad_of("feat"), "dqkv": _grad_of("qkv")}
    ops.update({k: _f(VEC) for k in vecs})
    return Op("front.conv_tail_norm_qkv[C=%d]" % C, "gcm", "gaussiancity_amd.front:conv_tail_norm_qkv", make, run, ops,
              {"lnc_eps": "a number", "ln1_eps": "a number"})


def _slots(gen, N, T):
    """order [T] and inverse [N] as get_padding_and_inverse makes them: every row has a slot, T - N rows a second one."""
    order = torch.cat([torch.randperm(N, generator=gen), torch.randperm(N, generator=gen)[:T - N]])
    inverse = torch.empty(N, dtype=torch.int64)
    inverse[order[:N]] = torch.arange(N)
    extra = torch.full((N,), -1, dtype=torch.int32)
    extra[order[N:]] = torch.arange(N, T, dtype=torch.int32)
    return order, inverse, extra


def _slot_plan():
    def make(gen):
        order, inverse, _ = _slots(gen, 65, 72)
        return {"order": order, "inverse": inverse}

    def run(t):
        from gaussiancity_amd import mid
        return {"extra": mid.slot_plan(t["order"], t["inverse"])}
    return Op("mid.slot_plan", "gcm", "gaussiancity_amd.mid:slot_plan", make, run, {"order": Operand(VEC), "inverse": Operand(VEC)},
              {"check": "a flag"})


def _gather_rows(W):
    def make(gen):
        order, inverse, extra = _slots(gen, 65, 72)
        return {"x": _randn(gen, 65, W), "order": order, "inverse": inverse, "extra": extra, "dy": _randn(gen, 72, W)}

    def run(t):
        from gaussiancity_amd import mid
        return {"y": mid.gather_rows(t["x"], t["order"], t["inverse"], t["extra"])}
    return Op("mid.gather_rows[W=%d]" % W, "gcm", "gaussiancity_amd.mid:gather_rows", make, run,
              {"x": _f(), "order": Operand(VEC), "inverse": Operand(VEC), "extra": Operand(VEC), "dy": _grad_of("y")})


def _proj_residual(C):
    def make(gen):
        _, inverse, extra = _slots(gen, 65, 72)
        return {"a": _randn(gen, 72, C), "inverse": inverse, "extra": extra, "x": _randn(gen, 65, C),
                "wp": _randn(gen, C, C, scale=C ** -0.5), "bp": _randn(gen, C),
                "row_scale": (torch.rand(65, generator=gen) < 0.7).float() / 0.7, "dy": _randn(gen, 65, C)}

    def run(t):
        from gaussiancity_amd import mid
        return {"y": mid.proj_residual(t["a"], t["inverse"], t["extra"], t["x"], t["wp"], t["bp"], t["row_scale"])}
    return Op("mid.proj_residual[C=%d]" % C, "gcm", "gaussiancity_amd.mid:proj_residual", make, run,
              {"a": _f(), "inverse": Operand(VEC), "extra": Operand(VEC), "x": _f(), "wp": _f(), "bp": _f(VECX),
               "row_scale": Operand(VECX), "dy": _grad_of("y")})


def _seam(I, training, product):
    N, O = 65, (48 if I > 4 else 8) if product else I

    def make(gen):
        return {"x": _randn(gen, N, I), "weight": _randn(gen, O, I, scale=I ** -0.5) if product else None,
                "bias": _randn(gen, O) if product else None, "bn_weight": _randn(gen, O), "bn_bias": _randn(gen, O),
                "running_mean": _randn(gen, O), "running_var": torch.rand(O, generator=gen) + 0.5,
                "num_batches_tracked": torch.tensor(3, dtype=torch.int64), "dy": _randn(gen, N, O)}

    def run(t):
        from gaussiancity_amd import seam
        return {"y": seam.linear_bn_gelu(t["x"], t["weight"], t["bias"], t["bn_weight"], t["bn_bias"], t["running_mean"],
                                         t["running_var"], t["num_batches_tracked"], training=training, momentum=0.1, eps=1e-5)}
    state = "inplace" if training else "in"
    ops = {"x": _f(), "bn_weight": _f(VEC), "bn_bias": _f(VEC), "running_mean": Operand(VEC, role=state),
           "running_var": Operand(VEC, role=state), "num_batches_tracked": Operand(VEC, role=state), "dy": _grad_of("y")}
    skipped = {"training": "a flag", "momentum": "a number", "eps": "a number", "act": "a flag"}
    if product:
        ops.update({"weight": _f(), "bias": _f(VECX)})
    else:
        skipped.update({"weight": "None in this entry: the chain without a product", "bias": "None without a weight"})
    return Op("seam.linear_bn_gelu[I=%d,%s,%s]" % (I, "training" if training else "eval", "weight" if product else "no weight"),
              "gcm", "gaussiancity_amd.seam:linear_bn_gelu", make, run, ops, skipped)


def _group(gen, N, G):
    return torch.randint(-1, G, (N,), generator=gen, dtype=torch.int32)


def _modulated_linear(I, O):
    N, G = 65, 3

    def make(gen):
        return {"x": _randn(gen, N, I), "weight": _randn(gen, O, I, scale=I ** -0.5), "alpha": _randn(gen, G, I), "beta": _randn(gen, G, O),
                "bias": _randn(gen, O), "group": _group(gen, N, G), "dy": _randn(gen, N, O)}

    def run(t):
        from gaussiancity_amd import modlinear
        return {"y": modlinear.modulated_linear(t["x"], t["weight"], t["alpha"], t["beta"], t["bias"], t["group"], 0.2)}
    return Op("modlinear.modulated_linear[I=%d,O=%d]" % (I, O), "gcm", "gaussiancity_amd.modlinear:modulated_linear", make, run,
              {"x": _f(), "weight": _f(), "alpha": _f(), "beta": _f(), "bias": _f(VECX), "group": Operand(VEC), "dy": _grad_of("y")},
              {"negative_slope": "a number"})


def _groups_from_masks():
    n = 130

    def make(gen):
        return {"masks.%d" % g: torch.rand(n, generator=gen) < 0.4 for g in range(3)}

    def run(t):
        from gaussiancity_amd import modlinear
        return {"group": modlinear.groups_from_masks([t["masks.%d" % g] for g in range(3)], n)}
    return Op("modlinear.groups_from_masks", "gcm", "gaussiancity_amd.modlinear:groups_from_masks", make, run,
              {"masks.%d" % g: Operand(VEC, param="masks") for g in range(3)}, {"n": "a number"})


def _head_out(I, kind, Cn):
    N = 65

    def make(gen):
        return {"f": _randn(gen, N, I), "weight": _randn(gen, Cn, I, scale=I ** -0.5), "bias": _randn(gen, Cn), "group": _group(gen, N, 3)}

    def run(t):
        from gaussiancity_amd import modlinear
        return {"out": modlinear.head_out(t["f"], t["weight"], t["bias"], t["group"], kind, 0.5)}
    return Op("modlinear.head_out[I=%d,%s]" % (I, kind), "gcm", "gaussiancity_amd.modlinear:head_out", make, run,
              {"f": Operand(MAT), "weight": Operand(MAT), "bias": Operand(VEC), "group": Operand(VEC)},
              {"kind": "a name", "factor": "a number"})


def _head_chain(I, H):
    N, K, G = 65, 5, 3
    shapes = {"x": (N, I), "onehots": (N, K), "w1": (H, I), "b1": (H,), "w_ma": (H, K), "w2": (H, H), "alpha": (G, H), "beta": (G, H),
              "bias2": (H,), "w_out": (3, H), "b_out": (3,)}

    def make(gen):
        c = {k: _randn(gen, *s, scale=0.3) for k, s in shapes.items()}
        c["group"] = _group(gen, N, G)
        return c

    def run(t):
        from gaussiancity_amd import modlinear
        return {"out": modlinear.head_chain(t["x"], t["onehots"], t["w1"], t["b1"], t["w_ma"], t["w2"], t["alpha"], t["beta"],
                                            t["bias2"], t["group"], t["w_out"], t["b_out"], "rgb", 1.0, 0.2)}
    ops = {k: Operand(MAT if len(s) == 2 else VEC) for k, s in shapes.items()}
    ops["group"] = Operand(VEC)
    return Op("modlinear.head_chain[I=%d,H=%d]" % (I, H), "gcm", "gaussiancity_amd.modlinear:head_chain", make, run, ops,
              {"kind": "a name", "factor": "a number", "negative_slope": "a number"})


_HEAD_KEYS = (("rgb", 3), ("opacity", 1), ("scale", 3))


def _head_train(I, packed):
    N = 65

    def make(gen):
        c = {}
        for kind, Cn in _HEAD_KEYS:
            c.update({"keys.%s.h" % kind: _randn(gen, N, I), "keys.%s.weight" % kind: _randn(gen, Cn, I, scale=I ** -0.5),
                      "keys.%s.bias" % kind: _randn(gen, Cn)})
        c["group"] = _group(gen, N, 3)
        if packed:
            c.update({"xyz": _randn(gen, N, 3), "scales": torch.rand((N, 3), generator=gen) + 0.5, "dpacked": _randn(gen, N, 14)})
        else:
            c.update({"d" + kind: _randn(gen, N, Cn) for kind, Cn in _HEAD_KEYS})
        return c

    def run(t):
        from gaussiancity_amd import modlinear
        keys = {kind: (t["keys.%s.h" % kind], t["keys.%s.weight" % kind], t["keys.%s.bias" % kind], 0.5) for kind, _ in _HEAD_KEYS}
        if packed:
            return {"packed": modlinear.head_points14(keys, t["xyz"], t["scales"], t["group"])}
        return modlinear.head_attrs(keys, t["group"])
    ops = {}
    for kind, _ in _HEAD_KEYS:
        ops.update({"keys.%s.h" % kind: _f(param="keys"), "keys.%s.weight" % kind: _f(param="keys"),
                    "keys.%s.bias" % kind: _f(VEC, param="keys")})
    ops["group"] = Operand(VEC)
    if packed:
        ops.update({"xyz": Operand(MAT), "scales": Operand(MAT), "dpacked": _grad_of("packed")})
    else:
        ops.update({"d" + kind: _grad_of(kind) for kind, _ in _HEAD_KEYS})
    name = "head_points14" if packed else "head_attrs"
    return Op("modlinear.%s[I=%d]" % (name, I), "gcm", "gaussiancity_amd.modlinear:" + name, make, run, ops)


# ---- libgca ----------------------------------------------------------------------------------------------------------------
_SEGMENTS = (1, 65, 0, 17)


def _attention(name, dtype, d):
    total, heads = sum(_SEGMENTS), 2

    def make(gen):
        cu = torch.tensor([0] + list(torch.tensor(_SEGMENTS).cumsum(0)), dtype=torch.int32)
        return {"qkv": _randn(gen, total, 3, heads, d).to(dtype), "cu_seqlens": cu, "dout": _randn(gen, total, heads, d).to(dtype)}

    def run(t):
        from gaussiancity_amd import attention
        return {"out": getattr(attention, name)(t["qkv"], t["cu_seqlens"], max(_SEGMENTS))}
    return Op("attention.%s[%s,d=%d]" % (name, str(dtype).split(".")[-1], d), "gca", "gaussiancity_amd.attention:" + name, make, run,
              {"qkv": _f(ND), "cu_seqlens": Operand(VEC), "dout": _grad_of("out", NDG)},
              {"max_seqlen": "a number", "softmax_scale": "a number"})


# ---- libgcs ----------------------------------------------------------------------------------------------------------------
def _voxels(gen, n, side=9, batches=2):
    """n distinct voxels of a [batches, side, side, side] grid, int32 [n, 4], in random order."""
    flat = torch.randperm(batches * side ** 3, generator=gen)[:n]
    b, r = flat // side ** 3, flat % side ** 3
    return torch.stack([b, r // side ** 2, r // side % side, r % side], 1).to(torch.int32)


def _engine(name):
    def setup(dev):
        from gaussiancity_amd import sparse
        prev = sparse.set_engine(name)
        return lambda: sparse.set_engine(prev)
    return setup


def _subm(cin, cout, dtype, engine):
    n = 300

    def make(gen):
        return {"features": _randn(gen, n, cin).to(dtype), "weight": _randn(gen, cout, 3, 3, 3, cin, scale=(27 * cin) ** -0.5).to(dtype),
                "bias": _randn(gen, cout).to(dtype), "indices": _voxels(gen, n), "dout": _randn(gen, n, cout).to(dtype)}

    def run(t):
        from gaussiancity_amd import sparse
        conv = sparse.SubMConv3d(cin, cout, 3, bias=True)
        del conv._parameters["weight"], conv._parameters["bias"]
        conv.weight, conv.bias = t["weight"], t["bias"]  # as they come: a view is no Parameter
        x = sparse.SparseConvTensor(t["features"], t["indices"], [9, 9, 9], 2)
        return {"out": conv(x).features}
    return Op("sparse.SubMConv3d[cin=%d,%s,%s]" % (cin, str(dtype).split(".")[-1], engine), "gcs", "gaussiancity_amd.sparse:SubMConv3d",
              make, run, {"features": _f(), "weight": _f(ND), "bias": _f(VECX), "indices": Operand(MAT), "dout": _grad_of("out")},
              setup=_engine(engine), parameters=("features", "indices", "weight", "bias"))


_INDPTR = (0, 1, 1, 40, 64, 130)


def _segment_csr(reduce, dtype, f):
    def make(gen):
        return {"src": _randn(gen, 130, f).to(dtype), "indptr": torch.tensor(_INDPTR), "out": torch.zeros(5, f, dtype=dtype),
                "dout": _randn(gen, 5, f).to(dtype)}

    def run(t):  # out= reaches the call only in the run that registers its refusal: the dense runs allocate their result
        from gaussiancity_amd import sparse
        out = t["out"] if t["out"].storage_offset() else None
        return {"out": sparse.segment_csr(t["src"], t["indptr"], out=out, reduce=reduce)}
    refused = Refuses("offset", NotImplementedError, "segment_csr(out=...) is not supported",
                      "the module takes no out= at all: the drop-in allocates its result")
    return Op("sparse.segment_csr[%s,%s,f=%d]" % (reduce, str(dtype).split(".")[-1], f), "gcs", "gaussiancity_amd.sparse:segment_csr",
            make, run, {"src": _f(), "indptr": Operand(VEC), "out": Operand((refused,)), "dout": _grad_of("out")}, {"reduce": "a name"})


def _codes(gen, k, n):
    return torch.randint(0, 1 << 12, (k, n), generator=gen, dtype=torch.int64)


def _pool_plan():
    def make(gen):
        return {"code": _codes(gen, 2, 130)}

    def run(t):
        from gaussiancity_amd import point_pool
        plan = point_pool.pool_plan(t["code"], 2)
        return {k: getattr(plan, k) for k in point_pool.FIELDS[:7]}
    return Op("point_pool.pool_plan", "gcs", "gaussiancity_amd.point_pool:pool_plan", make, run, {"code": Operand(MAT)},
              {"pooling_depth": "a number"})


_PLANS = {}


def _plan(dev):
    from gaussiancity_amd import point_pool
    key = str(dev)
    if key not in _PLANS:
        _PLANS[key] = point_pool.pool_plan(_codes(torch.Generator().manual_seed(21), 2, 130).to(dev), 2)
    return _PLANS[key]


def _pooled_reduce(reduce, dtype, f):
    def make(gen):
        s = int(torch.unique(_codes(torch.Generator().manual_seed(21), 2, 130)[0] >> 6).numel())
        return {"src": _randn(gen, 130, f).to(dtype), "dout": _randn(gen, s, f).to(dtype)}

    def run(t):
        from gaussiancity_amd import point_pool
        return {"out": point_pool.pooled_reduce(t["src"], _plan(t["src"].device), reduce)}
    return Op("point_pool.pooled_reduce[%s,%s,f=%d]" % (reduce, str(dtype).split(".")[-1], f), "gcs",
              "gaussiancity_amd.point_pool:pooled_reduce", make, run, {"src": _f(), "dout": _grad_of("out")},
              {"plan": "a PoolPlan, pool_plan's own dense result, not a caller's tensor", "reduce": "a name"})


def _unpool_add(dtype, f):
    def make(gen):
        s = int(torch.unique(_codes(torch.Generator().manual_seed(21), 2, 130)[0] >> 6).numel())
        return {"parent_feat": _randn(gen, 130, f).to(dtype), "child_feat": _randn(gen, s, f).to(dtype), "dout": _randn(gen, 130, f).to(dtype)}

    def run(t):
        from gaussiancity_amd import point_pool
        return {"out": point_pool.unpool_add(t["parent_feat"], t["child_feat"], _plan(t["child_feat"].device))}
    return Op("point_pool.unpool_add[%s,f=%d]" % (str(dtype).split(".")[-1], f), "gcs", "gaussiancity_amd.point_pool:unpool_add",
              make, run, {"parent_feat": _f(), "child_feat": _f(), "dout": _grad_of("out")},
              {"plan": "a PoolPlan, pool_plan's own dense result, not a caller's tensor"})


def _serialize():
    def make(gen):
        return {"grid_coord": torch.randint(0, 1 << 6, (130, 3), generator=gen, dtype=torch.int32),
                "batch": torch.randint(0, 2, (130,), generator=gen, dtype=torch.int64).sort().values}

    def run(t):
        from gaussiancity_amd import point_index
        code, order, inverse = point_index.serialize(t["grid_coord"], t["batch"], 6, ("z", "z-trans", "hilbert", "hilbert-trans"), n_batches=2)
        return {"code": code, "order": order, "inverse": inverse}
    return Op("point_index.serialize", "gcs", "gaussiancity_amd.point_index:serialize", make, run,
              {"grid_coord": Operand(MAT), "batch": Operand(VEC)},
              {"depth": "a number", "orders": "names", "grid_size": "a number", "n_batches": "a number"})


def _patch_plan():
    def make(gen):
        return {"offset": torch.tensor([1, 66, 66, 83, 213])}

    def run(t):
        from gaussiancity_amd import point_index
        pad, unpad, cu = point_index.patch_plan(t["offset"], 16)
        return {"pad": pad, "unpad": unpad, "cu_seqlens": cu}
    return Op("point_index.patch_plan", "gcs", "gaussiancity_amd.point_index:patch_plan", make, run, {"offset": Operand(VEC)},
              {"patch_size": "a number"})


# ---- libgcv: the image losses and the frame finish ---------------------------------------------------------------------------
_IMG = (37, 70)


def _l1():
    def make(gen):
        return {"a": torch.rand((2, 3) + _IMG, generator=gen), "b": torch.rand((2, 3) + _IMG, generator=gen),
                "mask": (torch.rand((2, 1) + _IMG, generator=gen) < 0.7).float(), "g": torch.tensor(0.75)}

    def run(t):
        from gaussiancity_amd import image_loss
        return {"loss": image_loss.l1(t["a"], t["b"], t["mask"])}
    return Op("image_loss.l1", "gcv", "gaussiancity_amd.image_loss:l1", make, run,
              {"a": _f(ND), "b": _f(ND), "mask": Operand(NDG, dim=0), "g": _grad_of("loss", VEC)})


def _gan_loss(real):
    def make(gen):
        label = torch.zeros((2, 8) + _IMG).scatter_(1, torch.randint(0, 8, (2, 1) + _IMG, generator=gen), 1.0)
        return {"pred": _randn(gen, 2, 9, *_IMG, scale=3.0), "label": label, "weight": torch.rand((2, 1) + _IMG, generator=gen),
                "g": torch.tensor(0.75)}

    def run(t):
        from gaussiancity_amd import image_loss
        return {"loss": image_loss.gan_loss(t["pred"], t["label"], t["weight"], real=real)}
    return Op("image_loss.gan_loss[real=%s]" % real, "gcv", "gaussiancity_amd.image_loss:gan_loss", make, run,
              {"pred": _f(ND), "label": Operand(ND), "weight": Operand(NDG, dim=0), "g": _grad_of("loss", VEC)}, {"real": "a flag"})


def _label_map():
    def make(gen):
        seg = torch.zeros((2, 8) + _IMG).scatter_(1, torch.randint(0, 8, (2, 1) + _IMG, generator=gen), 1.0)
        return {"seg": seg, "mask": (torch.rand((2, 1) + _IMG, generator=gen) < 0.7).float()}

    def run(t):
        from gaussiancity_amd import image_loss
        return {"label": image_loss.label_map(t["seg"], (9, 17), t["mask"])}
    return Op("image_loss.label_map", "gcv", "gaussiancity_amd.image_loss:label_map", make, run,
              {"seg": Operand(ND), "mask": Operand(NDG, dim=0)}, {"size": "two numbers"})


def _frame_finish():
    def make(gen):
        return {"img": torch.rand((3,) + _IMG, generator=gen) * 3 - 1.5, "ins_map": (torch.rand(_IMG, generator=gen) < 0.3).to(torch.int16)}

    def run(t):
        from gaussiancity_amd import finish
        out, u8 = finish.frame_finish(t["img"], t["ins_map"], 1)
        return {"image": out, "bytes": u8}
    return Op("finish.frame_finish", "gcv", "gaussiancity_amd.finish:frame_finish", make, run,
              {"img": Operand(ND), "ins_map": Operand(MAT)},
              {"road_id": "a number", "kernel_size": "a number", "sigma": "a number", "flip_mask_lr": "a flag", "want_float": "a flag",
               "want_uint8": "a flag", "bgr": "a flag"})


# ---- libgcv: generator inputs and the point volume ---------------------------------------------------------------------------
_SET = ("pts", "batch_idx", "instances", "classes", "scales")
_IDS = (1, 5, 6, 100, 101, 102, 207, 10000, 10003)  # KITTI-360: ground classes, facades and roofs, cars


def _visible(gen, m=130):
    """A visible set's five tensors (points.VisibleSet without its index), every instance of _IDS present."""
    ids = torch.tensor(_IDS, dtype=torch.int64)
    ins = ids[torch.cat([torch.randperm(len(ids), generator=gen), torch.randint(0, len(ids), (m - len(ids),), generator=gen)])]
    cls, bldg = ins.clone(), (ins >= 100) & (ins < 10000)
    cls[bldg & (ins % 2 == 0)], cls[bldg & (ins % 2 == 1)], cls[ins >= 10000] = 2, 7, 3
    pts = torch.cat([torch.randint(-300, 2300, (m, 3), generator=gen).float(), torch.randint(1, 5, (m, 1), generator=gen).float(),
                     ins.float()[:, None], torch.rand((m, 3), generator=gen) * 2 - 1], 1)
    return {"pts": pts.reshape(1, m, 8), "batch_idx": torch.searchsorted(ids, ins).to(torch.int32).reshape(1, m, 1),
            "instances": ids.to(torch.int16), "classes": cls.float().reshape(1, m, 1),
            "scales": (torch.rand((m, 3), generator=gen) * 1.6 + 0.4).reshape(1, m, 3)}


def _style(gen):
    lut = torch.zeros((max(_IDS) + 1, 12))
    has = torch.zeros((max(_IDS) + 1,), dtype=torch.uint8)
    for i in _IDS[3:]:
        lut[i], has[i] = torch.rand(12, generator=gen) * 2 - 1, 1
    return lut, has


def _split(t, lut, has):
    from gaussiancity_amd import model_inputs, points
    table = model_inputs.StyleTable({}, lut.device)
    table.lut, table.lut_has, table.n_lut, table.z_dim = lut, has, int(lut.shape[0]), int(lut.shape[1])
    vs = points.VisibleSet(None, *[t["visible_set." + k] for k in _SET])
    return model_inputs.split_by_model(vs, model_inputs.MODEL_RULE_KITTI_360(), table, proj_tlp=(3, -7))


def _split_by_model():
    def make(gen):
        c = {"visible_set." + k: v for k, v in _visible(gen).items()}
        c["style_table.lut"], c["style_table.lut_has"] = _style(gen)
        return c

    def run(t):
        split = _split(t, t["style_table.lut"], t["style_table.lut_has"])
        res = {"pts": split.pts, "scales": split.scales, "index": split.index}
        assert list(split.models) == ["BLDG", "CAR", "REST"]
        for name, m in split.models.items():
            res.update({"%s.%s" % (name, k): getattr(m, k) for k in ("batch_idx", "onehots", "proj_uv", "classes")})
            if m.zs is not None:
                res.update({"%s.zs.%s" % (name, k): getattr(m.zs, k) for k in ("group", "codes", "instances")})
        return res
    ops = {"visible_set." + k: Operand(ND if k != "instances" else VEC) for k in _SET}
    ops.update({"style_table.lut": Operand(VEC), "style_table.lut_has": Operand(VEC)})
    return Op("model_inputs.split_by_model", "gcv", "gaussiancity_amd.model_inputs:split_by_model", make, run, ops,
              {"model_rule": "a tuple of numbers", "proj_tlp": "two host values", "proj_size": "a number",
               "workspace": "a VisibleSetWorkspace: the module's own buffer, taken in 16-byte steps"})


_ATTRS = (("rgb", 3), ("xyz", 3), ("scale", 3), ("opacity", 1))


def _gaussian_points14():
    def rows(gen):
        ins = _visible(gen)["classes"].reshape(-1)
        return {"BLDG": int(((ins == 2) | (ins == 7)).sum()), "CAR": int((ins == 3).sum()), "REST": int(((ins != 2) & (ins != 7) & (ins != 3)).sum())}

    def make(gen):
        c = {"set." + k: v for k, v in _visible(torch.Generator().manual_seed(22)).items()}
        c["lut"], c["has"] = _style(torch.Generator().manual_seed(23))
        for name, n in rows(torch.Generator().manual_seed(22)).items():
            c.update({"attrs_per_model.%s.%s" % (name, k): _randn(gen, 1, n, w) for k, w in _ATTRS})
        return c

    def run(t):
        from gaussiancity_amd import model_inputs
        split = _split({"visible_set." + k: t["set." + k] for k in _SET}, t["lut"], t["has"])
        attrs = {name: {k: t["attrs_per_model.%s.%s" % (name, k)] for k, _ in _ATTRS} for name in split.models}
        return {"points14": model_inputs.gaussian_points14(split, attrs)}
    ops = {"attrs_per_model.%s.%s" % (name, k): Operand(ND) for name in ("BLDG", "CAR", "REST") for k, _ in _ATTRS}
    return Op("model_inputs.gaussian_points14", "gcv", "gaussiancity_amd.model_inputs:gaussian_points14", make, run, ops,
              {"split": "split_by_model's own result: tensors the module allocated"})


def _points_to_volume():
    n, dims = 130, (20, 24, 12)

    def make(gen):
        pts = torch.stack([torch.randint(0, d, (n,), generator=gen) for d in dims], 1).to(torch.int16)
        return {"points": pts, "pt_ids": torch.arange(1, n + 1, dtype=torch.int32)[torch.randperm(n, generator=gen)].reshape(n, 1),
                "scales": torch.randint(1, 4, (n, 1), generator=gen).to(torch.int16).repeat(1, 3)}

    def run(t):
        from gaussiancity_amd import points
        return {"volume": points.points_to_volume(t["points"], t["pt_ids"], t["scales"], *dims)}
    return Op("points.points_to_volume", "gcv", "gaussiancity_amd.points:points_to_volume", make, run,
              {"points": Operand(MAT), "pt_ids": Operand(MAT), "scales": Operand(MAT)},
              {"h": "a number", "w": "a number", "d": "a number", "return_occupancy": "a flag"})


def _visible_point_map():
    n, size = 650, 64

    def make(gen):
        xy = torch.randint(0, size, (n, 2), generator=gen)
        rows = torch.cat([xy, torch.randint(0, 20, (n, 1), generator=gen), torch.randint(1, 3, (n, 1), generator=gen),
                          torch.randint(1, 300, (n, 1), generator=gen)], 1).to(torch.int16)
        return {"rows": rows}

    def run(t):
        from gaussiancity_amd import points, synth
        rig, pos, quat = synth.layout_camera(size, W=70, H=37)
        vp_map, ins_map = points.visible_point_map(t["rows"], rig, pos.copy(), quat, 0)
        assert 0.05 < float((vp_map >= 0).float().mean()) < 1.0, "the case's camera must see some of the points and some sky"
        return {"vp_map": vp_map, "ins_map": ins_map}
    return Op("points.visible_point_map", "gcv", "gaussiancity_amd.points:visible_point_map", make, run, {"rows": Operand(MAT)},
              {"cam_rig": "host numbers", "cam_pos": "host numbers", "cam_quat": "host numbers", "null_class_id": "a number",
               "use_jumps": "a flag", "workspace": "a VolumeWorkspace: the module's own resident buffer"})


# ---- libgce ----------------------------------------------------------------------------------------------------------------
def _deterministic(mode):
    def setup(dev):
        from gaussiancity_amd import grid_encoder
        prev = grid_encoder._deterministic
        grid_encoder.set_deterministic(mode)
        return lambda: grid_encoder.set_deterministic(prev)
    return setup


def _grid_encoder(deterministic):
    D, L, C, B = 3, 3, 2, 257
    contiguous = "the binding's CHECK_CONTIGUOUS, as upstream's extension: ext_forward refuses a table that is not contiguous"

    def rows():
        from gaussiancity_amd import grid_encoder
        return grid_encoder.level_offsets(D, L, 2, 4, 8, False)[-1]

    def make(gen):
        return {"inputs": torch.rand((B, D), generator=gen) * 2 - 1, "embeddings": torch.rand((rows(), C), generator=gen) * 2 - 1,
                "dout": _randn(gen, B, L * C)}

    def run(t):
        from gaussiancity_amd import grid_encoder
        enc = grid_encoder.GridEncoder(D, L, C, 16, base_resolution=4, log2_hashmap_size=8).to(t["inputs"].device)
        del enc._parameters["embeddings"]
        enc.embeddings = t["embeddings"]
        return {"out": enc(t["inputs"])}

    def table_bar(case):
        """The table gradient under float atomics: every element within the summation bound of its own terms, the bar
        of tests/grid_rows.py (path "atomic")."""
        import numpy as np
        import grid_rows as GR
        from gaussiancity_amd import grid_encoder
        offsets = np.array(grid_encoder.level_offsets(D, L, 2, 4, 8, False), np.int64)
        unit = ((case["inputs"] + 1) / 2).numpy()  # GridEncoder.forward's arithmetic, float32
        grad = case["dout"].reshape(B, L, C).transpose(0, 1).contiguous().numpy()
        sum64, abs64, n = GR.terms_reference(grad, unit, int(offsets[-1]), offsets, 1.0, 4, 0, False, np.float32)
        bound = GR.hard_bound(n, abs64, sum64, GR.U[np.float32], GR.atomic_adds(n)) + GR.ref_bound(n, abs64)
        return torch.from_numpy(sum64), torch.from_numpy(bound)
    refused = [Refuses(k, RuntimeError, "embeddings must be a contiguous tensor", contiguous) for k in ("ragged_rows", "transposed")]
    return Op("grid_encoder.GridEncoder[%s]" % ("deterministic" if deterministic else "atomic"), "gce",
              "gaussiancity_amd.grid_encoder:GridEncoder", make, run,
              {"inputs": _f(), "embeddings": _f(["offset"] + refused), "dout": _grad_of("out")},
              setup=_deterministic(deterministic), parameters=("inputs", "embeddings"),
              bars=None if deterministic else {"grad:embeddings": table_bar})


# ---- the registry ----------------------------------------------------------------------------------------------------------
f16, f32 = torch.float16, torch.float32

REGISTRY = [
    _ffn(36, False), _ffn(36, True), _ffn(4, False), _ffn(4, True),
    _front(48), _front(4),
    _slot_plan(), _gather_rows(36), _gather_rows(4), _proj_residual(36), _proj_residual(4),
    _seam(36, True, True), _seam(36, False, True), _seam(48, True, False), _seam(48, False, False), _seam(4, True, True), _seam(4, False, True),
    _modulated_linear(36, 48), _modulated_linear(4, 4), _groups_from_masks(), _head_out(36, "rgb", 3), _head_out(4, "opacity", 1),
    _head_chain(36, 48), _head_chain(4, 4), _head_train(36, False), _head_train(4, False), _head_train(36, True), _head_train(4, True),
    _attention("varlen_qkvpacked", f16, 16), _attention("varlen_qkvpacked", f16, 64),
    _attention("varlen_attention", f32, 16), _attention("varlen_attention", f32, 64),
    _subm(6, 10, f32, "valu"), _subm(32, 36, f32, "valu"), _subm(6, 10, f32, "mfma"), _subm(32, 36, f32, "mfma"),
    _subm(6, 10, f16, "valu"), _subm(32, 36, f16, "valu"),
    _segment_csr("sum", f32, 36), _segment_csr("max", f32, 4), _segment_csr("mean", f16, 36),
    _pool_plan(), _pooled_reduce("sum", f32, 36), _pooled_reduce("mean", f32, 4), _pooled_reduce("min", f32, 36),
    _pooled_reduce("max", f16, 36), _unpool_add(f32, 36), _unpool_add(f16, 4),
    _serialize(), _patch_plan(),
    _l1(), _gan_loss(True), _gan_loss(False), _label_map(), _frame_finish(),
    _split_by_model(), _gaussian_points14(), _points_to_volume(), _visible_point_map(),
    _grid_encoder(True), _grid_encoder(False),
]
LIBRARIES = ("gcm", "gca", "gcs", "gcv", "gce")

# every operator the sweep answers for: a new one goes here and into REGISTRY
PUBLIC = tuple(sorted({op.target for op in REGISTRY}))


def registered_count():
    return sum(len(op.pairs()) for op in REGISTRY)
