"""The attribute head of the building generator over libgcm_hip.so (include/gcm.h):
GaussianAttrMLP.forward with style codes runs its ModLinear stack once per building instance -- a boolean-mask gather, a
modulated copy of the weight, three small products and a scatter each.  install() rebinds the method so that every
instance goes through ONE grouped product per layer (modlinear.modulated_linear): the number of launches does not depend
on the number of instances, and nothing waits for the device.

  install(generator) / uninstall(generator)   rebind GaussianAttrMLP.forward of a caller's imported models.generator
  stats() / reset_stats()                      calls that took the fused path, calls that went to the module's own method
  grouped_stats()                              fused calls whose zs was a model_inputs.GroupedCodes (no masks folded)
  install(generator, fused_outputs=True)       also the tail of a call with gradients -- fc_out, the transform and the
                                               uncovered rows of every key -- is one launch (modlinear.head_attrs), and a
                                               call with zs None (the background generator) and gradients ends in it too
  gaussian_points(mlp, pt_feat, onehots, zs, xyz, scales)     the same path ending in modlinear.head_points14: the
                                               rasterizer's [1, N, 14] without the dict and helpers.get_gaussian_points
  output_stats()                               calls that ended in head_attrs / head_points14

The module's own method runs, untouched, for zs None (the background generator; with fused_outputs and gradients only
what the plain path below does not take), CPU tensors, autocast or a dtype other than float32, a batch other than 1, a
layer that is not a ModLinear with output_mode=True, mod_bias=True, bias=None, and dimensions that are not multiples of 4.
"""
import torch

from . import modlinear
from .model_inputs import GroupedCodes

_STATS = {"fused_calls": 0, "original_calls": 0}
_GROUPED_STATS = {"grouped_calls": 0}  # beside stats(), whose two keys callers compare as a whole
_OUTPUT_STATS = {"head_attrs_calls": 0, "head_points14_calls": 0}
_ORIGINAL = "_gaussiancity_amd_attr_head_original"
_MOD_LINEAR = {}  # GaussianAttrMLP class of an installed module -> its ModLinear class, for gaussian_points


def stats():
    """Counters of this process: forwards that ran the fused kernels, forwards handed to the module's own method."""
    return dict(_STATS)


def grouped_stats():
    """Counter of this process: fused forwards whose zs was a model_inputs.GroupedCodes -- its group vector and code table
    were used as they are, without groups_from_masks and the torch.cat of the codes."""
    return dict(_GROUPED_STATS)


def output_stats():
    """Counters of this process: calls that ended in modlinear.head_attrs (forwards under install(fused_outputs=True) with
    gradients enabled) and in modlinear.head_points14 (gaussian_points)."""
    return dict(_OUTPUT_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0
    for k in _GROUPED_STATS:
        _GROUPED_STATS[k] = 0
    for k in _OUTPUT_STATS:
        _OUTPUT_STATS[k] = 0


def grouped_ok(zs, n):
    """zs is a GroupedCodes the kernels can take as it is: a contiguous int32 CUDA group vector of n rows and contiguous
    float32 CUDA codes."""
    group, codes = zs.group, zs.codes
    return (group.is_cuda and group.dtype == torch.int32 and tuple(group.shape) == (n,) and group.is_contiguous()
            and codes.is_cuda and codes.dtype == torch.float32 and codes.dim() == 2 and codes.is_contiguous())


def _layers(self):
    """(shared layers, {key: its layers}) in the order the method applies them."""
    first = self.n_shared_layers + 1
    shared = [getattr(self, "fc_%d" % i) for i in range(2, first)]
    own = {k: [getattr(self, "fc_%d_%s_%d" % (first, k, i)) for i in range(self.n_layers[k])] for k in self.factors.keys()}
    return shared, own


def _fusable(self, mod_linear, pt_feat, onehots, zs):
    if zs is None or len(zs) == 0 or torch.is_autocast_enabled():
        return False
    if not (pt_feat.is_cuda and onehots.is_cuda) or pt_feat.dtype != torch.float32 or onehots.dtype != torch.float32:
        return False
    if pt_feat.dim() != 3 or pt_feat.shape[0] != 1 or not isinstance(self.act, torch.nn.LeakyReLU):
        return False
    if not self.act.negative_slope > 0 or any(k not in modlinear.KINDS for k in self.factors.keys()):
        return False
    shared, own = _layers(self)
    for fc in shared + [fc for fcs in own.values() for fc in fcs]:
        if not isinstance(fc, mod_linear) or fc.bias is not None or not (fc.output_mode and fc.mod_bias):
            return False
        if fc.weight.dtype != torch.float32 or fc.weight.shape[0] % 4 or fc.weight.shape[1] % 4:
            return False
    if self.fc_1.weight.dtype != torch.float32 or self.fc_1.weight.shape[0] % 4:
        return False
    if isinstance(zs, GroupedCodes):
        return grouped_ok(zs, pt_feat.shape[1])
    return all(v["z"].dtype == torch.float32 and v["z"].is_cuda and v["idx"].dtype == torch.bool and v["idx"].is_cuda
               for v in zs.values())


def _fusable_plain(self, pt_feat, onehots):
    """A call with zs None whose output layers head_attrs / head_points14 can take: CUDA float32, batch 1, no autocast, a
    LeakyReLU of positive slope, every layer an nn.Linear(H, H), H a multiple of 4 within the library's limit."""
    if torch.is_autocast_enabled():
        return False
    if not (pt_feat.is_cuda and onehots.is_cuda) or pt_feat.dtype != torch.float32 or onehots.dtype != torch.float32:
        return False
    if pt_feat.dim() != 3 or pt_feat.shape[0] != 1 or not isinstance(self.act, torch.nn.LeakyReLU):
        return False
    if not self.act.negative_slope > 0 or any(k not in modlinear.KINDS for k in self.factors.keys()):
        return False
    H = self.fc_1.weight.shape[0]
    if self.fc_1.weight.dtype != torch.float32 or H % 4 or H > modlinear.head_train_limit():
        return False
    shared, own = _layers(self)
    for fc in shared + [fc for fcs in own.values() for fc in fcs]:
        if not isinstance(fc, torch.nn.Linear) or fc.weight.dtype != torch.float32 or tuple(fc.weight.shape) != (H, H):
            return False
    return all(getattr(self, "fc_out_%s" % k).weight.dtype == torch.float32 for k in self.factors.keys())


# ---- the method of models/generator.py, written against its behaviour: the first layer, the instances in dict order
# (a later instance's assignment wins where masks overlap), shared layers, then each key's layers, fc_out and the output
# transform; rows that no instance covers stay zeros ---------------------------------------------------------------------
def _hidden(self, pt_feat, onehots, zs):
    """The layers up to the shared activation, with style codes: (hidden, group), where hidden(key) runs the key's own
    layers and returns its last hidden activation [N, H] -- called key by key, so that without gradients only one key's
    activation is alive at a time."""
    n = pt_feat.shape[1]
    slope = self.act.negative_slope
    f = self.act(self.fc_1(pt_feat) + self.fc_m_a(onehots))[0]
    if isinstance(zs, GroupedCodes):  # the split already holds what the masks would be folded into
        group, codes = zs.group, zs.codes
        _GROUPED_STATS["grouped_calls"] += 1
    else:
        group = modlinear.groups_from_masks([v["idx"] for v in zs.values()], n)
        codes = torch.cat([v["z"].reshape(1, -1) for v in zs.values()])

    def layer(fc, h):
        alpha = torch.addmm(fc.bias_alpha, codes, fc.weight_alpha.t())
        beta = torch.addmm(fc.bias_beta, codes, fc.weight_beta.t())
        return modlinear.modulated_linear(h, fc.weight, alpha, beta, None, group, slope)

    shared, own = _layers(self)
    for fc in shared:
        f = layer(fc, f)

    def hidden(k):
        h = f
        for fc in own[k]:
            h = layer(fc, h)
        return h
    return hidden, group


def _hidden_plain(self, pt_feat, onehots):
    """The same for zs None, through the module's own layers.  Upstream applies each of a key's layers to the shared
    activation, not to the layer before it, so only the key's last layer reaches fc_out."""
    f = self.act(self.fc_1(pt_feat) + self.fc_m_a(onehots))[0]
    shared, own = _layers(self)
    for fc in shared:
        f = self.act(fc(f))
    return (lambda k: self.act(own[k][-1](f)) if own[k] else f), None


def _head_keys(self, hidden):
    keys = {}
    for k, factor in self.factors.items():
        fc_out = getattr(self, "fc_out_%s" % k)
        keys[k] = (hidden(k), fc_out.weight, fc_out.bias, factor)
    return keys


def _forward(original, mod_linear, fused_outputs=False):
    def forward(self, pt_feat, onehots, zs):
        """GaussianAttrMLP.forward with style codes over modlinear.modulated_linear."""
        grad = torch.is_grad_enabled()
        if fused_outputs and grad and zs is None and _fusable_plain(self, pt_feat, onehots):
            hidden, group = _hidden_plain(self, pt_feat, onehots)
            output = {k: v.unsqueeze(0) for k, v in modlinear.head_attrs(_head_keys(self, hidden), group).items()}
            _OUTPUT_STATS["head_attrs_calls"] += 1
            _STATS["fused_calls"] += 1
            return output
        if not _fusable(self, mod_linear, pt_feat, onehots, zs):
            _STATS["original_calls"] += 1
            return original(self, pt_feat, onehots, zs)
        hidden, group = _hidden(self, pt_feat, onehots, zs)
        if fused_outputs and grad and self.fc_1.weight.shape[0] <= modlinear.head_train_limit():
            output = {k: v.unsqueeze(0) for k, v in modlinear.head_attrs(_head_keys(self, hidden), group).items()}
            _OUTPUT_STATS["head_attrs_calls"] += 1
            _STATS["fused_calls"] += 1
            return output
        covered = (group >= 0).unsqueeze(1) if grad else None
        output = {}
        for k, factor in self.factors.items():
            h = hidden(k)
            fc_out = getattr(self, "fc_out_%s" % k)
            if not grad:
                output[k] = modlinear.head_out(h, fc_out.weight, fc_out.bias, group, k, factor).unsqueeze(0)
                continue
            v = fc_out(h)
            if k == "scale":
                v = 1 + v.clamp(-1, 1) * factor
            elif k == "opacity":
                v = torch.sigmoid(v) * factor + (1 - factor)
            else:
                v = (torch.sigmoid(v) - 0.5) * factor
            output[k] = torch.where(covered, v, torch.zeros((), dtype=v.dtype, device=v.device)).unsqueeze(0)
        _STATS["fused_calls"] += 1
        return output
    return forward


def gaussian_points(mlp, pt_feat, onehots, zs, xyz, scales):
    """The rasterizer's [1, N, 14] for a GaussianAttrMLP of an installed module: the layers as the rebound method runs them
    (style codes, or zs None through the module's own Linear layers), ending in modlinear.head_points14 -- what
    helpers.get_gaussian_points(xyz, scales, mlp(pt_feat, onehots, zs)) returns, without the dict, and with xyz and scales
    [1, N, 3] left as they are (they are data: no gradient).  Gradients reach pt_feat and the parameters.  A call the
    kernels cannot take raises ValueError: there is no other path here."""
    if type(mlp) not in _MOD_LINEAR:
        raise RuntimeError("gaussian_points needs attr_head.install() on the module that defines %s" % type(mlp).__name__)
    if "rgb" not in mlp.factors or mlp.fc_1.weight.shape[0] > modlinear.head_train_limit():
        raise ValueError("gaussian_points needs the rgb key and a hidden width within modlinear.head_train_limit()")
    if xyz.dim() != 3 or scales.dim() != 3 or xyz.shape[0] != 1 or scales.shape[0] != 1:
        raise ValueError("xyz and scales must be [1, N, 3]")
    if zs is None:
        if not _fusable_plain(mlp, pt_feat, onehots):
            raise ValueError("gaussian_points: this call (zs None) is not one the HIP output layers take")
        hidden, group = _hidden_plain(mlp, pt_feat, onehots)
    else:
        if not _fusable(mlp, _MOD_LINEAR[type(mlp)], pt_feat, onehots, zs):
            raise ValueError("gaussian_points: this call is not one the grouped kernels take")
        hidden, group = _hidden(mlp, pt_feat, onehots, zs)
    points = modlinear.head_points14(_head_keys(mlp, hidden), xyz[0], scales[0], group)
    _OUTPUT_STATS["head_points14_calls"] += 1
    return points.unsqueeze(0)


def install(generator_module, fused_outputs=False):
    """Rebind GaussianAttrMLP.forward of the caller's imported models.generator to the grouped kernels.  Idempotent;
    uninstall() puts the module's own method back.  fused_outputs: with gradients enabled the output layers of every key
    run in one launch (modlinear.head_attrs) instead of torch's fc_out, transform and where, and a call with zs None
    that fits (see _fusable_plain) takes that path too.  Off by default: the default is the behaviour without the option,
    bit for bit and launch for launch."""
    if getattr(generator_module, _ORIGINAL, None) is not None:
        return
    modlinear.dtypes()  # loads the library: a missing build fails here, not inside a forward
    original = generator_module.GaussianAttrMLP.forward
    setattr(generator_module, _ORIGINAL, original)
    _MOD_LINEAR[generator_module.GaussianAttrMLP] = generator_module.ModLinear
    generator_module.GaussianAttrMLP.forward = _forward(original, generator_module.ModLinear, bool(fused_outputs))


def uninstall(generator_module):
    original = getattr(generator_module, _ORIGINAL, None)
    if original is None:
        return
    generator_module.GaussianAttrMLP.forward = original
    _MOD_LINEAR.pop(generator_module.GaussianAttrMLP, None)
    delattr(generator_module, _ORIGINAL)
