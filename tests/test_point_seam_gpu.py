"""-m gpu: gaussiancity_amd.point_seam on the device, against the run of the reference's own
models/pt_v3.py that tests/golden/make_ptv3_seam_golden.py recorded (tests/golden/ptv3_seam.npz): one SerializedPooling +
SerializedUnpooling pair and one PointSequential(Linear, BatchNorm1d, GELU) on a Point, (a) in training mode and (b) in eval
mode on the state step (a) left.

With point_pool + point_seam installed on stand-in imports every recorded tensor -- the pooled and the unpooled feat, the
container's output, both input gradients, every parameter gradient and, for (a), the running statistics after the step --
is within 4 x the reference's float32 error of the reference's float64 run (the bar of the three fixtures before this one;
a bias gradient against the larger of its own maximum and its weight's, a buffer against its own maximum); the integer keys
and the counters are exact; the counters of point_seam show the fused path for the pooling tail, both unpooling chains and
the container.  With only point_seam installed the module's own pooling forward runs: its lone norm is one fused call
without the GELU, and the GELU is torch's.  One pass through a small whole PointTransformerV3 (tools/ptv3_stand_in.py:
two stages of widths 32 and 64, three Blocks) with point_pool, point_front, point_mid, point_ffn and point_seam composed,
in two install orders, agrees with the uninstalled run to the figures of tests/seam_ref.py's bar, and after uninstall bit
for bit (the forward and the buffers: torch's own index backward adds with float atomics).

Measured on the MI355X: with both installed the worst ratio of a tensor's error to the reference's float32 error is 1.97
(case b, the gradient of unpool.proj's BatchNorm weight, 4.0e-7 of its scale against 2.1e-7), under the bar of 4; the running
statistics after step (a) are at 1.00 to 1.65."""
import copy
import functools
import os
import types

import numpy as np
import pytest
import torch

from front_ref import FACTOR, FLOOR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BN = functools.partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ptv3_seam.npz"))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


class _Dict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


class _Sparse:
    """spconv.SparseConvTensor's features and replace_feature."""
    def __init__(self, features):
        self.features = features

    def replace_feature(self, features):
        return _Sparse(features)


def _stand_in():
    """What the installs need of models/pt_v3.py, written for this test from the modules' behaviour.  The pooling's own
    forward takes the clusters from the key `test_cluster` (the plan is point_pool's business, not this test's)."""
    class Point(_Dict):
        def sparsify(self, pad=96):
            self["sparse_conv_feat"] = _Sparse(self.feat)

    class PointModule(torch.nn.Module):
        pass

    class Conv(torch.nn.Module):
        """A spconv module's stand-in: maps the sparse tensor's features."""
        def __init__(self, cin, cout):
            super().__init__()
            self.lin = torch.nn.Linear(cin, cout, bias=False)

        def forward(self, s):
            return s.replace_feature(self.lin(s.features))

    spconv = types.SimpleNamespace(modules=types.SimpleNamespace(is_spconv_module=lambda m: isinstance(m, Conv)))

    class PointSequential(PointModule):
        """Upstream's constructor is (name="", *modules): a first module handed over positionally lands in `name`."""
        def __init__(self, name="", *modules):
            super().__init__()
            self.name = name
            for m in modules:
                self.add(m)

        def add(self, module):
            self.add_module(str(len(self._modules)), module)

        def forward(self, x):
            for module in self._modules.values():
                if isinstance(module, PointModule):
                    x = module(x)
                elif spconv.modules.is_spconv_module(module):
                    x.sparse_conv_feat = module(x.sparse_conv_feat)
                    x.feat = x.sparse_conv_feat.features
                elif isinstance(module, torch.nn.BatchNorm1d):
                    if x.feat.size(0) != 1:
                        x.feat = module(x.feat)
                else:
                    x.feat = module(x.feat)
                    if "sparse_conv_feat" in x.keys():
                        x.sparse_conv_feat = x.sparse_conv_feat.replace_feature(x.feat)
            return x

    class SerializedPooling(PointModule):
        def __init__(self, cin, cout, stride, norm_layer, act_layer, reduce, shuffle_orders, traceable=True):
            super().__init__()
            self.stride, self.reduce, self.shuffle_orders, self.traceable = stride, reduce, shuffle_orders, traceable
            self.proj = torch.nn.Linear(cin, cout)
            self.norm, self.act = PointSequential(norm_layer(cout)), PointSequential(act_layer())

        def forward(self, point):
            feat, cluster = self.proj(point.feat), point.test_cluster
            s = int(cluster.max()) + 1
            index = cluster[:, None].expand(-1, feat.shape[1])
            pooled = feat.new_full((s, feat.shape[1]), float("-inf")).scatter_reduce(0, index, feat, "amax")
            out = Point(feat=pooled, pooling_inverse=cluster, pooling_parent=point)
            if out.feat.size(0) != 1:
                out = self.norm(out)
            out = self.act(out)
            out.sparsify()
            return out

    class SerializedUnpooling(PointModule):
        def __init__(self, cin, cskip, cout, norm_layer, act_layer, traceable=False):
            super().__init__()
            self.proj = PointSequential(torch.nn.Linear(cin, cout), norm_layer(cout), act_layer())
            self.proj_skip = PointSequential(torch.nn.Linear(cskip, cout), norm_layer(cout), act_layer())
            self.traceable = traceable

        def forward(self, point):
            parent, inverse = point.pop("pooling_parent"), point.pop("pooling_inverse")
            point, parent = self.proj(point), self.proj_skip(parent)
            parent.feat = parent.feat + point.feat[inverse]
            return parent

    return types.SimpleNamespace(Point=Point, PointModule=PointModule, PointSequential=PointSequential, Conv=Conv, spconv=spconv,
                                 SerializedPooling=SerializedPooling, SerializedUnpooling=SerializedUnpooling)


def _modules(M, gold, dev, case):
    pool = M.SerializedPooling(20, 36, int(gold["stride"]), BN, torch.nn.GELU, str(gold["reduce"]), False)
    unpool = M.SerializedUnpooling(36, 20, 12, BN, torch.nn.GELU)
    seq = M.PointSequential(torch.nn.Linear(20, 28), BN(28), torch.nn.GELU())
    mods = {"pool": pool, "unpool": unpool, "seq": seq}
    for name, module in mods.items():
        state = {k: torch.from_numpy(gold["w.%s.%s" % (name, k)]) for k in module.state_dict()}
        if case == "b":     # eval mode after one training step: the state the reference's step (a) left
            for k in state:
                if k.endswith(("running_mean", "running_var")):
                    state[k] = torch.from_numpy(gold["a.buf.%s.%s" % (name, k)]).float()
                elif k.endswith("num_batches_tracked"):
                    state[k] = torch.from_numpy(gold["a.int.buf.%s.%s" % (name, k)])
        module.load_state_dict(state)
        module.to(dev).train(case == "a")
    return mods


def _run(dev, M, gold, case, own_pooling=False):
    mods = _modules(M, gold, dev, case)
    t = lambda k: torch.from_numpy(gold[k]).to(dev)  # noqa: E731
    g = lambda k: t("%s.int.%s" % (case, k))  # noqa: E731
    feat, feat_seq = t("feat").requires_grad_(True), t("feat").requires_grad_(True)
    common = dict(coord=t("coord"), grid_coord=t("grid"), batch=t("batch"), grid_size=float(gold["grid_size"]))
    point = M.Point(feat=feat, serialized_code=g("in.serialized_code"), serialized_order=g("in.serialized_order"),
                    serialized_inverse=g("in.serialized_inverse"), serialized_depth=int(gold["%s.int.in.serialized_depth" % case]),
                    test_cluster=g("pooling_inverse"), **common)
    before = {"%s.%s" % (name, k): b.clone() for name, m in mods.items() for k, b in m.named_buffers()}
    pooled = mods["pool"](point)
    ints = {} if own_pooling else {k: pooled[k].cpu().numpy() for k in (
        "grid_coord", "serialized_code", "serialized_order", "serialized_inverse", "batch", "pooling_inverse")}
    floats = {"pooled": pooled.feat}
    assert torch.equal(pooled.sparse_conv_feat.features, pooled.feat)
    parent = mods["unpool"](pooled)
    floats["unpooled"] = parent.feat
    out = mods["seq"](M.Point(feat=feat_seq, **common))
    floats["seq"] = out.feat
    params = [("%s.%s" % (name, k), p) for name, module in mods.items() for k, p in module.named_parameters()]
    loss = (parent.feat * t("dout")).sum() + (out.feat * t("dseq")).sum()
    grads = torch.autograd.grad(loss, [feat, feat_seq] + [p for _, p in params])
    floats["grad.feat"], floats["grad.feat_seq"] = grads[0], grads[1]
    for (name, _), gr in zip(params, grads[2:]):
        floats["grad." + name] = gr
    for name, module in mods.items():
        for k, b in module.named_buffers():
            key = "buf.%s.%s" % (name, k)
            if b.dtype == torch.int64:
                ints[key] = b.cpu().numpy()
            elif case == "a":
                floats[key] = b
            else:
                assert torch.equal(b, before["%s.%s" % (name, k)]), key      # eval mode leaves the running statistics alone
    return ints, {k: v.detach().double().cpu().numpy() for k, v in floats.items()}


def _compare(gold, case, ints, floats, only=None):
    for k, v in ints.items():
        assert np.array_equal(v, gold["%s.int.%s" % (case, k)]), k
    worst = []
    for name, value in floats.items():
        if only is not None and name not in only:
            continue
        want, err32 = gold["%s.%s" % (case, name)], float(gold["%s.err32.%s" % (case, name)])
        err = float(np.abs(value - want).max() / float(gold["%s.scale.%s" % (case, name)]))
        print("%s %-40s %.2e of the scale, the reference's float32 run %.2e, ratio %.2f" % (case, name, err, err32, err / err32))
        if not err <= 4 * err32:
            worst.append((name, err, err32))
    assert not worst, worst


@pytest.mark.parametrize("case", ["a", "b"])
def test_pool_and_seam_installed_match_the_reference_run(dev, golden, case):
    from gaussiancity_amd import point_pool, point_seam, seam
    M = _stand_in()
    point_pool.install(M)
    point_seam.install(M)
    try:
        point_seam.reset_stats()
        seam.reset_stats()
        ints, floats = _run(dev, M, golden, case)
        st, lib = point_seam.stats(), seam.stats()
    finally:
        point_seam.uninstall(M)
        point_pool.uninstall(M)
    # the pooling tail, the two unpooling chains and the container: four runs, one of them the tail; nothing else ran
    assert st == {"fused_runs": 4, "pooling_tails": 1, "original_modules": 0, "original_calls": 0}, st
    assert lib == {"forward_train_calls": 4 * (case == "a"), "forward_eval_calls": 4 * (case == "b"), "backward_calls": 4}, lib
    recorded = {k[2:] for k in golden.files if k.startswith(case + ".") and k.split(".")[1] in ("pooled", "unpooled", "seq", "grad", "buf")}
    assert set(floats) == recorded
    _compare(golden, case, ints, floats)


@pytest.mark.parametrize("case", ["a", "b"])
def test_with_only_seam_installed_the_modules_own_pooling_runs_its_norm_fused_and_its_gelu_in_torch(dev, golden, case):
    from gaussiancity_amd import point_seam
    M = _stand_in()
    point_seam.install(M)
    try:
        point_seam.reset_stats()
        ints, floats = _run(dev, M, golden, case, own_pooling=True)
        st = point_seam.stats()
    finally:
        point_seam.uninstall(M)
    # the lone norm, the two unpooling chains and the container are runs; the act container has no norm: the module's own
    assert st == {"fused_runs": 4, "pooling_tails": 0, "original_modules": 0, "original_calls": 1}, st
    _compare(golden, case, ints, floats)


def _whole_pass(model, frame, dout, dev, dtype):
    model = copy.deepcopy(model).to(device=dev, dtype=dtype)
    data = {k: (v.to(device=dev, dtype=dtype) if v.is_floating_point() else v.to(dev)) for k, v in frame.items()}
    data["feat"].requires_grad_(True)
    out = model(data)
    (out.feat * dout.to(device=dev, dtype=dtype)).sum().backward()
    res = {"y": out.feat, "dx": data["feat"].grad}
    res.update({"d." + k: p.grad for k, p in model.named_parameters()})
    res.update({"b." + k: b for k, b in model.named_buffers() if b.is_floating_point()})
    return {k: v.detach().cpu() for k, v in res.items()}


@pytest.mark.parametrize("order", ("pool, front, mid, ffn, seam", "seam, ffn, mid, front, pool"))
def test_a_small_whole_backbone_with_every_install_agrees_with_the_uninstalled_run(dev, order):
    """tools/ptv3_stand_in.py's PointTransformerV3, two stages of widths 32 and 64 (stem, Block, pooling, Block, unpooling,
    Block), training mode, 600 rows in 3 batch elements: one forward + backward with the five installs composed."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ptv3_stand_in as S
    from gaussiancity_amd import point_ffn, point_front, point_mid, point_pool, point_seam
    mods = {"pool": point_pool, "front": point_front, "mid": point_mid, "ffn": point_ffn, "seam": point_seam}
    M = S.NAMESPACE
    torch.manual_seed(11)
    model = S.PointTransformerV3(cin=8, widths=(32, 64), depth=8).train()
    frame = S.sloped_frame(600, 3, 8, cin=8)
    dout = torch.randn(600, 64)
    want = _whole_pass(model, frame, dout, "cpu", torch.float64)
    yard = _whole_pass(model, frame, dout, dev, torch.float32)
    names = order.split(", ")
    try:
        for name in names:
            mods[name].install(M)
        for m in mods.values():
            m.reset_stats()
        got = _whole_pass(model, frame, dout, dev, torch.float32)
        st = {name: m.stats() for name, m in mods.items()}
    finally:
        for name in list(reversed(names)) + names:
            mods[name].uninstall(M)
    assert not [n for n in vars(M) if n.startswith("_gaussiancity_amd")]
    again = _whole_pass(model, frame, dout, dev, torch.float32)
    # the stem's tail, the pooling tail and both unpooling chains are one call each; the stem's convolution is the one
    # module the walk ran itself; the three Blocks took the fused front, middle and tail
    assert st["seam"]["fused_runs"] == 4 and st["seam"]["pooling_tails"] == 1 and st["seam"]["original_modules"] == 1, st["seam"]
    assert st["pool"]["pooling_fused"] == 1 and st["pool"]["unpooling_fused"] == 1, st["pool"]
    assert st["front"]["fused_calls"] == 3 and st["mid"]["fused_calls"] == 3 and st["ffn"]["fused_calls"] == 3, st
    # after uninstall: the bits of a run that never installed (the forward and the buffers; torch's own index backward adds
    # with float atomics and has no bits to compare)
    assert all(torch.equal(again[k], yard[k]) for k in yard if k == "y" or k.startswith("b."))
    failed = []
    for k in want:
        scale = want[k].abs().max()
        if k.endswith(".bias") and k.startswith("d."):    # in front of batch statistics a bias has the gradient 0
            scale = max(scale, want[k[:-4] + "weight"].abs().max())
        e_got = float((got[k].double() - want[k]).abs().max() / scale)
        e_yard = float((yard[k].double() - want[k]).abs().max() / scale)
        bar = max(FACTOR * e_yard, FLOOR)
        print("%-44s operator %.3e  torch float32 %.3e  ratio %.2f  bar %.3e" % (k, e_got, e_yard, e_got / max(e_yard, 1e-30), bar))
        if not e_got <= bar:
            failed.append((k, e_got, bar))
    assert not failed, failed
