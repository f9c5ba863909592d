"""The operand-view sweep's table is complete, its view builders build what they claim, and the layout helper the
wrappers share does what the sweep relies on.  No GPU: signatures, CPU tensors."""
import importlib
import inspect

import pytest
import torch

import operand_views as OV
from gaussiancity_amd._loader import dense, fresh

# the operators the sweep answers for
OPERATORS = """
ffn:layernorm_mlp_residual front:conv_tail_norm_qkv mid:slot_plan mid:gather_rows mid:proj_residual seam:linear_bn_gelu
modlinear:modulated_linear modlinear:groups_from_masks modlinear:head_out modlinear:head_chain modlinear:head_attrs
modlinear:head_points14 attention:varlen_qkvpacked attention:varlen_attention sparse:SubMConv3d sparse:segment_csr
point_pool:pool_plan point_pool:pooled_reduce point_pool:unpool_add point_index:serialize point_index:patch_plan
image_loss:l1 image_loss:gan_loss image_loss:label_map finish:frame_finish grid_encoder:GridEncoder
model_inputs:split_by_model model_inputs:gaussian_points14 points:points_to_volume points:visible_point_map
""".split()

# what else those modules export that takes an argument, and why the sweep has no entry for it
_NUMBERS = "takes numbers or names, no tensor"
_INSTALL = "rebinds a caller's module; the operators it installs are in the table"
_RAW = "the extension's raw entry point, reached through GridEncoder; refuses a tensor that is not contiguous, as upstream's"
_TORCH = "the torch formulation the HIP operator is checked against"
_OUTSIDE = "a voxel-library or host-side entry point outside this sweep's list of operators"
OTHERS = {
    "ffn:split_plan": _NUMBERS, "finish:gaussian_kernel2d": _NUMBERS, "grid_encoder:set_deterministic": _NUMBERS,
    "grid_encoder:level_offsets": _NUMBERS, "sparse:set_engine": _NUMBERS, "sparse:engine_products": _NUMBERS,
    "model_inputs:MODEL_RULE_GOOGLE_EARTH": _NUMBERS, "model_inputs:MODEL_RULE_KITTI_360": _NUMBERS,
    "sparse:is_spconv_module": "takes a module", "sparse:SparseModule": "the empty base class of SubMConv3d",
    "finish:road_blur": "frame_finish with one of its two results chosen: the same checks and the same launch",
    "image_loss:GANLoss": "the module over gan_loss", "model_inputs:style_table": "converts a host dict, on the host",
    "grid_encoder:ext_forward": _RAW, "grid_encoder:ext_backward": _RAW, "grid_encoder:ext_backward_deterministic": _RAW,
    "image_loss:torch_l1": _TORCH, "image_loss:torch_gan_loss": _TORCH, "image_loss:torch_label_map": _TORCH,
    "image_loss:install": _INSTALL, "image_loss:uninstall": _INSTALL, "point_index:install": _INSTALL,
    "point_index:uninstall": _INSTALL, "point_pool:install": _INSTALL, "point_pool:uninstall": _INSTALL,
    "point_pool:gather_forward": "the call under pooled_reduce, which the sweep reaches through it",
    "point_pool:gather_backward": "the call under pooled_reduce's backward, which the sweep reaches through it",
    "points:extrude_points": _OUTSIDE, "points:get_points_from_projection": _OUTSIDE, "points:maps_to_volume": _OUTSIDE,
    "points:ray_voxel_intersection_perspective": _OUTSIDE, "points:centers_table": _OUTSIDE, "points:visible_point_set": _OUTSIDE,
    "points:get_camera_look_at": _OUTSIDE, "points:get_visible_points": _OUTSIDE,
}

DTYPES = (torch.float32, torch.float16, torch.int32, torch.int64, torch.bool, torch.uint8)


def _short(target):
    return target.replace("gaussiancity_amd.", "")


def test_the_registry_holds_the_operators_and_nothing_else():
    assert sorted(_short(t) for t in OV.PUBLIC) == sorted(OPERATORS)
    ids = [op.id for op in OV.REGISTRY]
    assert len(set(ids)) == len(ids)
    assert {op.lib for op in OV.REGISTRY} == set(OV.LIBRARIES)


def test_every_export_of_the_operator_modules_is_an_entry_or_has_a_reason():
    """A new operator without an entry fails here: every public function with a parameter, and every torch module class,
    that an operator module defines is in the table or in OTHERS."""
    missing = []
    for name in sorted({t.split(":")[0] for t in OPERATORS}):
        mod = importlib.import_module("gaussiancity_amd." + name)
        for attr, obj in vars(mod).items():
            if attr.startswith("_") or getattr(obj, "__module__", None) != mod.__name__:
                continue
            operator = (inspect.isfunction(obj) and len(inspect.signature(obj).parameters) > 0) or (
                inspect.isclass(obj) and issubclass(obj, torch.nn.Module))
            key = "%s:%s" % (name, attr)
            if operator and key not in OPERATORS and key not in OTHERS:
                missing.append(key)
    assert not missing, "no entry in tests/operand_views.py and no reason in OTHERS: %s" % ", ".join(missing)
    stale = [k for k in OTHERS if not hasattr(importlib.import_module("gaussiancity_amd." + k.split(":")[0]), k.split(":")[1])]
    assert not stale, stale


@pytest.mark.parametrize("op", OV.REGISTRY, ids=[op.id for op in OV.REGISTRY])
def test_every_parameter_is_swept_or_has_a_reason(op):
    """Every parameter of the public signature has operands with at least the offset view, or a named reason."""
    parameters = op.parameters()
    public = op.public()
    if inspect.isclass(public):  # the names given with the entry are the module's parameters and the entry's own operands
        module_parameters = {"sparse:SubMConv3d": {"weight", "bias"}, "grid_encoder:GridEncoder": {"embeddings"}}[_short(op.target)]
        assert module_parameters <= set(parameters) and set(parameters) <= set(op.operands)
        source = inspect.getsource(public)
        assert all("self.%s = torch.nn.Parameter" % p in source for p in module_parameters)
    for p in parameters:
        operands = op.covered(p)
        if not operands:
            assert op.skipped.get(p), "%s: parameter %s has no operand in the table and no reason" % (op.id, p)
            continue
        assert p not in op.skipped, (op.id, p)
        for name, o in operands.items():
            assert "offset" in [OV._kind_name(k) for k in o.kinds], "%s: %s lacks the offset view" % (op.id, name)
    assert set(op.skipped) <= set(parameters), "%s: reasons for parameters the signature does not have" % op.id
    assert all(o.param is None or o.param in parameters for o in op.operands.values())


@pytest.mark.parametrize("op", OV.REGISTRY, ids=[op.id for op in OV.REGISTRY])
def test_every_registered_view_builds_on_the_entrys_case(op):
    """Nothing can drop out at run time: the case has every operand, every kind applies to its shape, gradients name an
    output, a refusal names its error and its reason."""
    case = op.make(torch.Generator().manual_seed(20))
    again = op.make(torch.Generator().manual_seed(20))
    assert all(OV.bits_equal(case[k], again[k]) for k in case if isinstance(case[k], torch.Tensor)), "the case is seeded"
    assert len(op.pairs()) >= len(op.operands) > 0
    for name, o in op.operands.items():
        assert isinstance(case.get(name), torch.Tensor), "%s: the case has no %s" % (op.id, name)
        assert o.role in ("in", "grad", "inplace") and (o.role != "grad" or o.of)
        assert len({OV._kind_name(k) for k in o.kinds}) == len(o.kinds) > 0
        for k in o.kinds:
            if isinstance(k, OV.Refuses):
                assert k.kind in OV.KINDS and issubclass(k.error, Exception) and k.message and k.why
            else:
                assert k in OV.KINDS
            built = OV.build(OV._kind_name(k), case[name], o.dim)
            assert built.view.shape == case[name].shape


def test_the_count_is_the_tables():
    assert OV.registered_count() == sum(len(o.kinds) for op in OV.REGISTRY for o in op.operands.values()) > 500


# ---- the builders ------------------------------------------------------------------------------------------------------
def _values(dtype, *shape):
    n = 1
    for s in shape:
        n *= s
    return (torch.arange(n) % 5 + 1).reshape(shape).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[-1] for d in DTYPES])
def test_builders_build_what_they_claim(dtype):
    t = _values(dtype, 65, 36)
    size = t.element_size()
    off = OV.build("offset", t)
    assert off.view.is_contiguous() and off.view.data_ptr() % 16 == size and off.view.data_ptr() - off.base.data_ptr() == size
    assert size != 2 or off.view.data_ptr() % 4 == 2
    assert off.base.numel() == t.numel() + 2 and off.outside().numel() == 2 and torch.equal(off.view, t)
    for shape in ((36,), ()):  # a parameter vector, a 0-d counter
        v = OV.build("offset", _values(dtype, *shape))
        assert v.view.shape == shape and v.view.data_ptr() % 16 == size
    rag = OV.build("ragged_rows", t)
    assert rag.view.stride() == (37, 1) and rag.view.storage_offset() == 1 and not rag.view.is_contiguous()
    assert rag.outside().numel() == 65 and torch.equal(rag.view, t)
    assert OV.build("ragged_rows", _values(dtype, 65, 3)).view.stride() == (5, 1)  # 3 + 1 would be a multiple of 4
    assert OV.build("ragged_rows", _values(dtype, 2, 3, 5, 8)).view.stride() == (135, 45, 9, 1)
    tr = OV.build("transposed", t)
    assert tr.view.stride() == (1, 65) and torch.equal(tr.view, t) and not tr.filler
    ex = OV.build("expanded", t)
    assert ex.view.stride() == (0, 0) and ex.base.numel() == 1 and torch.equal(ex.view, t[:1, :1].expand(65, 36))
    ex0 = OV.build("expanded", t, 0)
    assert ex0.view.stride() == (0, 1) and torch.equal(ex0.view, t[:1].expand(65, 36))
    for b in (off, rag):  # the filler is the filler, in the buffer's dtype, and only there
        assert bool((b.outside() == torch.tensor(OV.FILL).to(dtype)).all())
        b.view.zero_()
        assert bool((b.outside() == torch.tensor(OV.FILL).to(dtype)).all()) and not bool(b.take(b.base).any())


def test_bits_equal_tells_bits_apart():
    a = torch.tensor([0.0, float("nan"), 1.0])
    assert OV.bits_equal(a, a.clone()) and not OV.bits_equal(a, torch.tensor([-0.0, float("nan"), 1.0]))
    assert not OV.bits_equal(a, a.double()) and not OV.bits_equal(a, a[:2]) and OV.bits_equal(None, None) and not OV.bits_equal(a, None)


# ---- the layout helper of the wrappers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[-1] for d in DTYPES])
def test_dense_returns_a_dense_aligned_tensor_of_equal_values(dtype):
    t = _values(dtype, 65, 36)
    assert t.data_ptr() % 16 == 0
    assert dense(t) is t, "the dense aligned path gains no copy"
    whole = t.view(-1)
    assert dense(whole) is whole
    for kind in OV.KINDS:
        v = OV.build(kind, t).view
        d = dense(v)
        assert d is not v and d.is_contiguous() and d.data_ptr() % 16 == 0 and d.stride() == (36, 1), kind
        assert d.dtype == dtype and OV.bits_equal(d, v.contiguous()), kind
    v = OV.build("offset", _values(dtype, 36)).view
    assert v.contiguous() is v or v.contiguous().data_ptr() == v.data_ptr(), "contiguous() leaves an offset view where it is"
    assert dense(v).data_ptr() % 16 == 0 and torch.equal(dense(v), v)
    assert dense(v, align=t.element_size()) is v, "an operand whose library asks for element alignment stays in place"
    f = fresh(t)
    assert f is not t and f.data_ptr() != t.data_ptr() and f.stride() == t.stride() and torch.equal(f, t)


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[-1] for d in DTYPES])
def test_dense_of_no_rows_is_empty(dtype):
    buf = _values(dtype, 40)
    for empty in (buf[1:1].view(0, 4), buf[:0].view(0, 4), torch.empty((0, 4), dtype=dtype), torch.empty((0, 4), dtype=dtype).t()):
        d = dense(empty)
        assert d.shape == empty.shape and d.numel() == 0 and d.dtype == dtype and d.is_contiguous()
