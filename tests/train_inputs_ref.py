"""What core/train.py:207-224 computes between the data loader and the generator, restated in torch on the CPU in this
project's words: the yardstick of gaussiancity_amd.train_inputs.  Every value is an integer or one rounded float32
operation, so the comparisons are bit for bit.

  restate(pts, rule, z_dim, proj_tlp)   dict of bch_idx, classes, scales, onehots, proj_uv, and with a z_dim the keys,
                                        codes [I, z_dim] and masks [I, N] of get_z -- drawn from the default CPU generator
  flagged(pts, rule)                    bool [B, N]: the rows the device flags (upstream asserts on them, on the host or in
                                        scatter_); their one-hot row is zero and their group -1, every other value is the
                                        formula's
  groups(pts, rule)                     (group int32 [N], ids int16 [I]) of a [1, N, 9] crop
"""
import torch

MAX_INSTANCE = 32768


def classes_of(instances, rule):
    """The class of an instance id: three masks taken from the ids, assigned in the order facade, roof, car."""
    in_bldg = (instances >= rule.bldg_ins_min) & (instances < rule.bldg_ins_max)
    facade, roof = in_bldg & (instances % 2 == 0), in_bldg & (instances % 2 == 1)
    car = (instances >= rule.car_ins_min) & (instances < rule.car_ins_max)
    classes = instances.clone()
    classes[facade] = rule.facade_class
    classes[roof] = rule.roof_class
    classes[car] = rule.car_class
    return classes


def scales_of(scale, classes, rule):
    """[B,N,1] * SCALE_FACTOR on three axes, z = 1 where the class is special."""
    s = (scale * rule.scale_factor).repeat(1, 1, 3)
    special = torch.isin(classes[..., 0], torch.tensor(list(rule.special_z_classes), dtype=torch.int64))
    s[..., 2][special] = 1
    return s


def flagged(pts, rule):
    ins = pts[:, :, 4]
    cls = classes_of(ins, rule)
    ok_ins = (ins >= 0) & (ins < MAX_INSTANCE) & (ins == ins.floor())
    ok_cls = (cls >= 0) & (cls < rule.n_classes) & (cls == cls.floor())
    return ~(ok_ins & ok_cls)


def one_hot(classes, n_classes, bad):
    """scatter_(2, classes.long(), 1) on zeros, as a comparison; a flagged row stays zero."""
    hot = classes == torch.arange(n_classes, dtype=torch.float32)
    return (hot & ~bad.unsqueeze(-1)).float()


def proj_uv_of(abs_xyz, proj_tlp, proj_size):
    uv = abs_xyz[..., :2].clone() if proj_tlp is None else abs_xyz[..., :2] - torch.as_tensor(proj_tlp).unsqueeze(1)
    uv[..., 0] /= proj_size
    uv[..., 1] /= proj_size
    return uv * 2 - 1


def groups(pts, rule):
    ins = pts[0, :, 4]
    bad = flagged(pts, rule)[0]
    ids = torch.unique(ins[(ins >= 0) & (ins < MAX_INSTANCE) & (ins == ins.floor())])
    group = torch.searchsorted(ids, ins.clamp(0, MAX_INSTANCE - 1).nan_to_num(0.0)).to(torch.int32)
    group[bad] = -1
    return group, ids.to(torch.int16)


def draw_codes(instances, z_dim):
    """get_z: the distinct ids ascending, one torch.randn(1, z_dim) each from the default generator, one mask each."""
    assert instances.shape[0] == 1 and instances.shape[2] == 1
    keys = [int(i) for i in torch.unique(instances).short()]
    codes = [torch.randn(1, z_dim) for _ in keys]
    masks = [instances[..., 0] == k for k in keys]
    return keys, torch.cat(codes), torch.cat(masks)


def restate(pts, rule, z_dim=None, proj_tlp=None):
    pts = pts.detach().cpu()
    instances = pts[:, :, 4:5]
    classes = classes_of(instances, rule)
    bad = flagged(pts, rule)
    out = {"bch_idx": pts[:, :, 8].long(), "classes": classes, "scales": scales_of(pts[:, :, 3:4], classes, rule),
           "onehots": one_hot(classes, rule.n_classes, bad), "proj_uv": proj_uv_of(pts[:, :, :3], proj_tlp, rule.proj_size),
           "flagged": int(bad.sum())}
    if z_dim is not None:
        out["z_keys"], out["z_codes"], out["z_idx"] = draw_codes(instances, z_dim)
    return out
