"""-m gpu: the head's output layers in a training step (gcm_head_train_* through modlinear.head_attrs / head_points14;
DESIGN.md section 17c).  The forward has head_out's bits per key and helpers.get_gaussian_points' in the [N, 14] form; the
backward is held to the float64 reference on the stored pre (tests/head_train_ref.py: cases, bars, the direct caller), for
both gradient forms, and is the same from run to run, on another stream and over a workspace full of NaN.

Shapes: N around the 16-row block of the forward and the 64-row tile of the backward; I = 4, 52 (a short walk of the
64-stride), 68 (a ragged one) and 512 (the real reduction length); two large N at I = 8 taken from the plan."""
import numpy as np
import pytest
import torch

from head_train_ref import KINDS, N_GROUPS, N_TWO_TILES, PRE_AT, channels, hold, library_plan, make_case, run_raw
from modlinear_ref import head_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


NS, IS = (1, 15, 16, 17, 63, 64, 65, 333), (4, 52, 68, 512)


def _tensors(dev, c, need=("h", "w", "b"), h_extra=0):
    """{kind: (h, weight, bias, factor)} as leaves on the device."""
    keys = {}
    for kind in c["kinds"]:
        k = c["keys"][kind]
        h = torch.from_numpy(k["h"]).to(dev)
        if h_extra:
            wide = torch.zeros((h.shape[0], h.shape[1] + h_extra), device=dev)
            wide[:, :h.shape[1]] = h
            h = wide[:, :h.shape[1]]
        h = h.requires_grad_("h" in need)
        w = torch.from_numpy(k["w"]).to(dev).requires_grad_("w" in need)
        b = None if k["b"] is None else torch.from_numpy(k["b"]).to(dev).requires_grad_("b" in need)
        keys[kind] = (h, w, b, k["factor"])
    return keys


def _group(dev, c):
    return None if c["group"] is None else torch.from_numpy(c["group"]).to(dev)


def _autograd(dev, c, packed, need=("h", "w", "b"), h_extra=0, dp_extra=0, retain=False):
    """head_attrs / head_points14 and one backward: out.<kind> or p14, and dh / dw / db per key, as numpy."""
    from gaussiancity_amd import modlinear
    keys = _tensors(dev, c, need, h_extra)
    res = {}
    if packed:
        xyz, scales = torch.from_numpy(c["xyz"]).to(dev), torch.from_numpy(c["scales"]).to(dev)
        p = modlinear.head_points14(keys, xyz, scales, _group(dev, c))
        assert torch.equal(xyz.cpu(), torch.from_numpy(c["xyz"])) and torch.equal(scales.cpu(), torch.from_numpy(c["scales"]))
        res["p14"] = p.detach().cpu().numpy()
        dp = torch.from_numpy(c["dp"]).to(dev)
        if dp_extra:
            wide = torch.full((dp.shape[0], 14 + dp_extra), 7.0, device=dev)
            wide[:, :14] = dp
            dp, seen = wide[:, :14], []
            p.register_hook(lambda g: seen.append(g.stride()))
        p.backward(dp, retain_graph=retain)
        assert not dp_extra or seen == [dp.stride()], "autograd handed the backward another dP than the strided one"
        again = (lambda: p.backward(dp)) if retain else None
    else:
        out = modlinear.head_attrs(keys, _group(dev, c))
        assert list(out) == list(c["kinds"])
        res.update({"out." + k: v.detach().cpu().numpy() for k, v in out.items()})
        douts = [torch.from_numpy(c["keys"][k]["dout"]).to(dev) for k in c["kinds"]]
        torch.autograd.backward(list(out.values()), douts, retain_graph=retain)
        again = (lambda: torch.autograd.backward(list(out.values()), douts)) if retain else None
    for kind, (h, w, b, _) in keys.items():
        for name, t in (("dh", h), ("dw", w), ("db", b)):
            if t is not None and t.requires_grad:
                res["%s.%s" % (name, kind)] = t.grad.cpu().numpy().copy()
            elif t is not None:
                assert t.grad is None
    return (res, keys, again) if retain else res


def _same(a, b, names=None):
    names = [n for n in a if n in b] if names is None else names
    assert names
    return [n for n in names if a[n].tobytes() != b[n].tobytes()]


# ---- forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", IS)
@pytest.mark.parametrize("N", NS)
def test_forward_has_the_bits_of_head_out_per_key(dev, N, I):
    from gaussiancity_amd import modlinear
    for bias in (True, False):
        for group in (None, "mixed", "bare"):
            c = make_case(N, I, ("rgb", "opacity", "xyz", "scale"), seed=N * 1000 + I, bias=bias, group=group)
            keys, g = _tensors(dev, c, need=()), _group(dev, c)
            out = modlinear.head_attrs(keys, g)
            alone = modlinear.head_attrs({"opacity": keys["opacity"]}, g)["opacity"]
            for kind, (h, w, b, factor) in keys.items():
                want = modlinear.head_out(h, w, b, g, kind, factor)
                assert out[kind].dtype == torch.float32 and tuple(out[kind].shape) == (N, channels(kind))
                assert out[kind].cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (kind, bias, group)
                if group == "bare":
                    assert not out[kind].any()
            assert torch.equal(alone, out["opacity"])
            if group == "mixed" and bias:  # and head_out itself is where the float64 reference puts it
                for kind in c["kinds"]:
                    k = c["keys"][kind]
                    _, want, bar = head_reference(kind, k["h"], k["w"], k["b"], k["factor"])
                    live = c["group"] >= 0
                    assert (np.abs(out[kind].cpu().numpy() - want)[live] <= bar[live]).all(), kind


@pytest.mark.parametrize("kinds", [("rgb",), ("scale", "rgb"), ("xyz", "rgb", "scale", "opacity")])
@pytest.mark.parametrize("N,I", [(1, 4), (17, 52), (65, 68), (333, 512)])
def test_points14_is_get_gaussian_points_on_the_per_key_values(dev, N, I, kinds):
    from gaussiancity_amd import helpers, modlinear
    for group in (None, "mixed"):
        c = make_case(N, I, kinds, seed=N + I, group=group)
        keys, g = _tensors(dev, c, need=()), _group(dev, c)
        xyz, scales = torch.from_numpy(c["xyz"]).to(dev), torch.from_numpy(c["scales"]).to(dev)
        wide = torch.full((N, 5), 9.0, device=dev)   # scales as a view of wider rows
        wide[:, :3] = scales
        p = modlinear.head_points14(keys, xyz, wide[:, :3], g)
        assert tuple(p.shape) == (N, 14) and p.dtype == torch.float32
        assert torch.equal(xyz.cpu(), torch.from_numpy(c["xyz"])) and torch.equal(wide[:, :3].cpu(), torch.from_numpy(c["scales"]))
        attrs = {k: v.unsqueeze(0) for k, v in modlinear.head_attrs(keys, g).items()}
        want = helpers.get_gaussian_points(xyz.clone().unsqueeze(0), scales.clone().unsqueeze(0), attrs)[0]
        assert p.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (kinds, group)
        got = p.cpu().numpy()
        assert (got[:, 7] == 1).all() and not got[:, 8:11].any()
        if "opacity" not in kinds:
            assert (got[:, 3] == 1).all()
        if "xyz" not in kinds:
            assert got[:, 0:3].tobytes() == c["xyz"].tobytes()
        if "scale" not in kinds:
            assert got[:, 4:7].tobytes() == c["scales"].tobytes()


# ---- backward -----------------------------------------------------------------------------------------------------------
def _check_backward(dev, c, packed, label):
    raw = run_raw(dev, c, packed_out=packed, packed_grad=packed)
    got = _autograd(dev, c, packed)
    assert not _same(raw, got), _same(raw, got)   # the autograd layer hands on what the library wrote
    dvs = hold(c, got, raw["pre"], packed, label)
    return raw, got, dvs


@pytest.mark.parametrize("packed", [False, True], ids=["dict", "points14"])
@pytest.mark.parametrize("I", IS)
@pytest.mark.parametrize("N", NS)
def test_backward_within_the_bars(dev, N, I, packed):
    c = make_case(N, I, KINDS, seed=7 * N + I, bias=True, group="mixed")
    raw, got, dvs = _check_backward(dev, c, packed, "N%d I%d" % (N, I))
    if N >= 15:
        pre = raw["pre"][:, PRE_AT["scale"]:PRE_AT["scale"] + 3]
        live = c["group"] >= 0
        inside = (pre >= -1) & (pre <= 1)
        assert (inside & live[:, None]).any() and (~inside & live[:, None]).any(), "the clamp must be active and inactive"
        assert (pre[1] == 1.0).all() and (pre[2] == -1.0).all() and live[1] and live[2]
        assert (dvs["scale"][1:3] != 0).all() and got["dh.scale"][1:3].any(axis=1).all()   # pre = +-1 passes the gradient
        assert (c["group"] < 0).any() and not got["dh.rgb"][c["group"] < 0].any()


@pytest.mark.parametrize("packed", [False, True], ids=["dict", "points14"])
def test_backward_without_bias_and_without_group(dev, packed):
    for bias, group in ((False, "mixed"), (True, None), (False, None)):
        c = make_case(65, 68, ("rgb", "scale"), seed=3, bias=bias, group=group)
        _, got, _ = _check_backward(dev, c, packed, "bias %s group %s" % (bias, group))
        assert ("db.rgb" in got) == bias


def test_a_whole_tile_and_every_row_without_a_group(dev):
    c = make_case(200, 52, KINDS, seed=5, group="mixed")
    c["group"][64:128] = -1
    _, got, _ = _check_backward(dev, c, False, "tile 1 bare")
    assert not got["dh.xyz"][64:128].any()
    c = make_case(70, 8, KINDS, seed=6, group="bare")
    _, got, _ = _check_backward(dev, c, True, "all bare")
    assert all(not got[n].any() for n in got if n[:2] in ("dh", "dw", "db"))


@pytest.mark.parametrize("N,branch", [(N_GROUPS, "groups"), (N_TWO_TILES, "two tiles per block")])
def test_the_plans_of_many_rows(dev, N, branch):
    """I = 8: 14 fold groups of 3 records behind a short last tile; and row blocks that walk two tiles, the last of them
    one, over two fold levels."""
    p = library_plan(N, 8)
    assert N % 64 and p["groups"] >= 2 and p["levels"] == 2 and (p["tpb"] == 2 and p["tiles"] % 2 == 1 if branch != "groups" else p["tpb"] == 1)
    c = make_case(N, 8, ("rgb", "opacity"), seed=N, group="mixed")
    _check_backward(dev, c, True, branch)


def test_two_keys_that_share_one_h(dev):
    from gaussiancity_amd import modlinear
    c = make_case(130, 52, ("rgb", "scale"), seed=9, group="mixed")
    c["keys"]["scale"]["h"] = c["keys"]["rgb"]["h"].copy()
    raw = run_raw(dev, c)
    keys = _tensors(dev, c)
    h = keys["rgb"][0]
    keys["scale"] = (h,) + keys["scale"][1:]
    out = modlinear.head_attrs(keys, _group(dev, c))
    torch.autograd.backward(list(out.values()), [torch.from_numpy(c["keys"][k]["dout"]).to(dev) for k in c["kinds"]])
    assert h.grad.cpu().numpy().tobytes() == (raw["dh.rgb"] + raw["dh.scale"]).tobytes()
    assert keys["scale"][1].grad.cpu().numpy().tobytes() == raw["dw.scale"].tobytes()


def test_strided_h_and_strided_dp_give_the_contiguous_bits(dev):
    c = make_case(130, 52, KINDS, seed=10, group="mixed")
    dense = _autograd(dev, c, True)
    assert not _same(dense, _autograd(dev, c, True, h_extra=8, dp_extra=2))
    assert not _same(dense, run_raw(dev, c, packed_out=True, packed_grad=True, h_extra=12, dp_extra=6))
    assert not _same(_autograd(dev, c, False), _autograd(dev, c, False, h_extra=4))


def test_bits_do_not_depend_on_the_run_the_stream_or_what_memory_held(dev):
    c = make_case(N_GROUPS, 8, KINDS, seed=11, group="mixed")
    for packed in (False, True):
        first = run_raw(dev, c, packed_out=packed, packed_grad=packed)
        assert not any(np.isnan(v).any() for v in first.values() if v is not first["pre"])
        assert not _same(first, run_raw(dev, c, packed_out=packed, packed_grad=packed))
        side = torch.cuda.Stream()
        assert not _same(first, run_raw(dev, c, packed_out=packed, packed_grad=packed, stream=side))
        filled = run_raw(dev, c, packed_out=packed, packed_grad=packed, nan_fill=True)
        assert not _same(first, filled, [n for n in first if n != "pre"])
        used = [PRE_AT[k] + i for k in c["kinds"] for i in range(channels(k))]
        assert first["pre"][:, used].tobytes() == filled["pre"][:, used].tobytes()


# ---- edges --------------------------------------------------------------------------------------------------------------
def test_no_rows(dev):
    c = make_case(0, 8, ("rgb", "opacity"), seed=1, group=None)
    for packed in (False, True):
        got = _autograd(dev, c, packed)
        assert got["dh.rgb"].shape == (0, 8) and not got["dw.rgb"].any() and not got["db.opacity"].any()
        raw = run_raw(dev, c, packed_out=packed, packed_grad=packed, nan_fill=True)
        assert not raw["dw.opacity"].any() and not raw["db.rgb"].any()


def test_retain_graph_and_a_second_backward(dev):
    c = make_case(65, 52, ("rgb", "scale"), seed=12, group="mixed")
    for packed in (False, True):
        once, keys, again = _autograd(dev, c, packed, retain=True)
        again()
        for kind, (h, w, b, _) in keys.items():   # the second backward wrote the same bits: grad = g + g
            assert h.grad.cpu().numpy().tobytes() == (once["dh." + kind] * 2).tobytes()
            assert w.grad.cpu().numpy().tobytes() == (once["dw." + kind] * 2).tobytes()
            assert b.grad.cpu().numpy().tobytes() == (once["db." + kind] * 2).tobytes()


def test_an_input_that_asks_for_no_gradient_gets_no_tensor(dev):
    from gaussiancity_amd import modlinear
    c = make_case(65, 52, ("rgb", "opacity"), seed=13, group="mixed")
    full = _autograd(dev, c, False)
    for need, counts in ((("w",), (0, 2, 0)), (("h",), (2, 0, 0)), (("b",), (0, 0, 2)), (("h", "b"), (2, 0, 2))):
        modlinear.reset_stats()
        got = _autograd(dev, c, False, need=need)
        s = modlinear.head_train_stats()
        assert (s["dh_outputs"], s["dw_outputs"], s["db_outputs"]) == counts and s["forward_calls"] == s["backward_calls"] == 1
        assert not _same(got, full) and len([n for n in got if n[:2] in ("dh", "dw", "db")]) == sum(counts)


def test_what_python_refuses(dev):
    from gaussiancity_amd import modlinear
    c = make_case(17, 8, ("rgb", "scale"), seed=14)
    keys = _tensors(dev, c)
    xyz, scales = torch.from_numpy(c["xyz"]).to(dev), torch.from_numpy(c["scales"]).to(dev)
    with pytest.raises(ValueError, match="must not require"):
        modlinear.head_points14(keys, xyz.clone().requires_grad_(True), scales)
    with pytest.raises(ValueError, match="must not require"):
        modlinear.head_points14(keys, xyz, scales.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="rgb"):
        modlinear.head_points14({"scale": keys["scale"]}, xyz, scales)
    with pytest.raises(ValueError, match="kind"):
        modlinear.head_attrs({"colour": keys["rgb"]})
    with pytest.raises(ValueError, match="weight"):
        modlinear.head_attrs({"opacity": keys["rgb"]})
    with pytest.raises(ValueError, match="multiple of 4"):
        modlinear.head_attrs({"rgb": (torch.zeros(4, 516, device=dev), torch.zeros(3, 516, device=dev), None, 1.0)})
