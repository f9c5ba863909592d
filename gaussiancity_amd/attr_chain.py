"""The attribute head at inference in one launch per output key over libgcm_hip.so (include/gcm.h, gcm_head_chain;
DESIGN.md section 17b): under no_grad GaussianAttrMLP.forward needs none of its hidden activations in memory, so fc_1,
fc_m_a, the activation, the key's hidden layer, fc_out and the output transform run as ONE kernel per key
(modlinear.head_chain) -- for the background generator (zs None, plain Linear layers) and for the building generator (style
codes, one ModLinear per key; every instance in the same launch through the group vector of attr_head).

  install(generator) / uninstall(generator)   rebind GaussianAttrMLP.forward of a caller's imported models.generator
  stats() / reset_stats()                      forwards that took the chain, forwards passed on to the method bound before
  grouped_stats()                              chained forwards whose zs was a model_inputs.GroupedCodes (no masks folded)

A second layer beside attr_head, installed separately: attr_head keeps the calls with gradients (and its counters).  The
method that sees a call first is the one installed last, so install attr_chain after attr_head for the chain to take the
building generator's no_grad calls.  Either may be uninstalled first.  (attr_head.uninstall puts the module's own method
back: when it runs while attr_chain is bound over it, the chain goes with it; uninstall() here then only drops its marker
and install() binds again.)

The chain takes a call when gradients are disabled, autocast is off, the tensors are CUDA float32, act is a LeakyReLU with
a positive slope, n_shared_layers is 1, every key is one of modlinear.KINDS, the widths are multiples of 4 within the
library's caps, and either zs is None and every key has at least one layer, all nn.Linear(H, H), or zs is what attr_head
accepts (batch 1, boolean masks, float32 codes) and every key has exactly one ModLinear(output_mode=True, mod_bias=True,
bias=None).  Every other call goes, untouched and counted, to the method that was bound before.

With zs None upstream applies every layer of a key to f, not to the layer before it, so only the key's LAST layer reaches
fc_out: that is the layer the chain runs.  With codes a later instance wins where masks overlap.
"""
import torch

from . import attr_head, modlinear
from .model_inputs import GroupedCodes

_STATS = {"chain_calls": 0, "passed_on_calls": 0}
_GROUPED_STATS = {"grouped_calls": 0}  # beside stats(), whose two keys callers compare as a whole
_ORIGINAL = "_gaussiancity_amd_attr_chain_original"
_BOUND = "_gaussiancity_amd_attr_chain_bound"


def stats():
    """Counters of this process: forwards that ran the chained kernel, forwards handed to the method bound before."""
    return dict(_STATS)


def grouped_stats():
    """Counter of this process: chained forwards whose zs was a model_inputs.GroupedCodes -- its group vector and code
    table were used as they are, without groups_from_masks and the torch.cat of the codes."""
    return dict(_GROUPED_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0
    for k in _GROUPED_STATS:
        _GROUPED_STATS[k] = 0


def _f32(t):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32


def _plan(self, mod_linear, pt_feat, onehots, zs):
    """None, or {key: the hidden layer the chain runs for it} when the chain takes this call."""
    if torch.is_grad_enabled() or torch.is_autocast_enabled():
        return None
    if not (_f32(pt_feat) and _f32(onehots)) or pt_feat.dim() != 3 or onehots.dim() != 3:
        return None
    if pt_feat.shape[:2] != onehots.shape[:2] or not isinstance(self.act, torch.nn.LeakyReLU) or not self.act.negative_slope > 0:
        return None
    if self.n_shared_layers != 1 or any(k not in modlinear.KINDS for k in self.factors.keys()):
        return None
    fc_1, fc_m_a = self.fc_1, self.fc_m_a
    if not (isinstance(fc_1, torch.nn.Linear) and isinstance(fc_m_a, torch.nn.Linear)) or fc_1.bias is None or fc_m_a.bias is not None:
        return None
    (H, I), K = fc_1.weight.shape, fc_m_a.weight.shape[1]
    max_in, max_hidden = modlinear.head_chain_limits()
    if H % 4 or I % 4 or H > max_hidden or I > max_in or not 1 <= K <= 32 or fc_m_a.weight.shape[0] != H:
        return None
    if pt_feat.shape[2] != I or onehots.shape[2] != K or not (_f32(fc_1.weight) and _f32(fc_m_a.weight)):
        return None
    plan = {}
    for k in self.factors.keys():
        layers = [getattr(self, "fc_2_%s_%d" % (k, i), None) for i in range(self.n_layers[k])]
        fc_out = getattr(self, "fc_out_%s" % k)
        if not isinstance(fc_out, torch.nn.Linear) or tuple(fc_out.weight.shape) != (1 if k == "opacity" else 3, H):
            return None
        if not layers or not _f32(fc_out.weight) or any(getattr(fc, "weight", None) is None for fc in layers):
            return None
        if any(tuple(fc.weight.shape) != (H, H) or not _f32(fc.weight) for fc in layers):
            return None
        if zs is None:
            if not all(isinstance(fc, torch.nn.Linear) for fc in layers):
                return None
        else:
            fc = layers[0]
            if len(layers) != 1 or not isinstance(fc, mod_linear) or fc.bias is not None or not (fc.output_mode and fc.mod_bias):
                return None
        plan[k] = layers[-1]
    if zs is not None:
        if len(zs) == 0 or pt_feat.shape[0] != 1:
            return None
        if isinstance(zs, GroupedCodes):
            return plan if attr_head.grouped_ok(zs, pt_feat.shape[1]) else None
        if not all(_f32(v["z"]) and v["idx"].dtype == torch.bool and v["idx"].is_cuda for v in zs.values()):
            return None
    return plan


def _forward(original, generator_module):
    def forward(self, pt_feat, onehots, zs):
        """GaussianAttrMLP.forward under no_grad over modlinear.head_chain: one launch per key."""
        plan = None
        if getattr(generator_module, _BOUND, None) is forward:  # else: uninstalled while another binding holds this method
            plan = _plan(self, generator_module.ModLinear, pt_feat, onehots, zs)
            if plan is None:
                _STATS["passed_on_calls"] += 1
        if plan is None:
            return original(self, pt_feat, onehots, zs)
        b, n, I = pt_feat.shape
        x, hot = pt_feat.reshape(b * n, I), onehots.reshape(b * n, onehots.shape[2])
        slope = self.act.negative_slope
        group = codes = None
        if isinstance(zs, GroupedCodes):  # the split already holds what the masks would be folded into
            group, codes = zs.group, zs.codes
            _GROUPED_STATS["grouped_calls"] += 1
        elif zs is not None:
            group = modlinear.groups_from_masks([v["idx"] for v in zs.values()], n)
            codes = torch.cat([v["z"].reshape(1, -1) for v in zs.values()])
        output = {}
        for k, factor in self.factors.items():
            fc, fc_out = plan[k], getattr(self, "fc_out_%s" % k)
            alpha = beta = bias2 = None
            if zs is None:
                bias2 = fc.bias
            else:
                alpha = torch.addmm(fc.bias_alpha, codes, fc.weight_alpha.t())
                beta = torch.addmm(fc.bias_beta, codes, fc.weight_beta.t())
            out = modlinear.head_chain(x, hot, self.fc_1.weight, self.fc_1.bias, self.fc_m_a.weight, fc.weight, alpha, beta,
                                       bias2, group, fc_out.weight, fc_out.bias, k, factor, slope)
            output[k] = out.reshape(b, n, out.shape[1])
        _STATS["chain_calls"] += 1
        return output
    return forward


def install(generator_module):
    """Rebind GaussianAttrMLP.forward of the caller's imported models.generator to the chained kernel, over whatever is
    bound now (attr_head's method when that is installed).  Idempotent while its method is the one bound, directly or under
    attr_head's; uninstall() puts back what it found."""
    bound = getattr(generator_module, _BOUND, None)
    head = generator_module.GaussianAttrMLP
    if bound is not None and (head.forward is bound or getattr(generator_module, attr_head._ORIGINAL, None) is bound):
        return
    modlinear.head_chain_limits()  # loads the library: a build without the operator fails here, not inside a forward
    original = head.forward
    bound = _forward(original, generator_module)
    setattr(generator_module, _ORIGINAL, original)
    setattr(generator_module, _BOUND, bound)
    head.forward = bound


def uninstall(generator_module):
    """Put back the method install() found, if GaussianAttrMLP.forward is still install()'s.  When attr_head was installed
    over it, attr_head is told to restore that method instead; when the method is neither's, only the marker goes."""
    bound = getattr(generator_module, _BOUND, None)
    if bound is None:
        return
    original = getattr(generator_module, _ORIGINAL)
    if generator_module.GaussianAttrMLP.forward is bound:
        generator_module.GaussianAttrMLP.forward = original
    elif getattr(generator_module, attr_head._ORIGINAL, None) is bound:
        setattr(generator_module, attr_head._ORIGINAL, original)
    for name in (_ORIGINAL, _BOUND):
        delattr(generator_module, name)
