"""A sequential numpy formulation of scripts/inference.py:239-256, written from upstream's behaviour: the three masks of
_get_pt_indexes_by_models, per model the boolean-mask gathers and the renumbering loop of _get_pt_attrs_by_models (as a
loop), _get_z as a dict, get_one_hot, get_projection_uv in float32 in upstream's order, the per-key concatenation and
get_gaussian_points.  tests/golden/model_inputs.npz (the reference's own lines, recorded) holds it to the reference."""
import numpy as np

MODELS = ("BLDG", "CAR", "REST")
F32 = np.float32


def model_of_class(class_ids, n_classes, bldg=True, car=True, rest=True):
    """int8 [32]: the model slot per class.  class_ids: {"BLDG_FACADE", "BLDG_ROOF", "CAR" (optional)} -> class id.
    An absent BLDG / CAR model sends its classes to REST (_get_pt_indexes_by_models); an absent REST model drops its rows."""
    t = np.full(32, -1, np.int8)
    t[:n_classes] = 2 if rest else -1
    if bldg:
        t[[class_ids["BLDG_FACADE"], class_ids["BLDG_ROOF"]]] = 0
    if car and "CAR" in class_ids:
        t[class_ids["CAR"]] = 1
    return t


def get_z(instances, lut):
    """_get_z: instances float [n]; lut {id: code [z_dim]}.  None, or {id: {"z": [1, z_dim], "idx": bool [1, n]}}."""
    unique = [int(np.int16(v)) for v in np.unique(instances)]
    unique_z = {ui: lut[ui] for ui in unique if ui in lut}
    if not unique_z:
        return None
    return {ui: {"z": np.asarray(unique_z[ui], F32).reshape(1, -1), "idx": (instances == ui)[None]} for ui in unique if ui in unique_z}


def groups_of(zs, n):
    """The group vector attr_head folds the dict's masks into: the largest g whose mask has the row, -1 where none has."""
    group = np.full(n, -1, np.int32)
    for g, v in enumerate(zs.values()):
        group[v["idx"][0]] = g
    return group


def projection_uv(xy, tlp, proj_size):
    uv = xy.copy() if tlp is None else xy - np.asarray(tlp).astype(F32)[None]
    uv = uv / F32(proj_size)
    return uv * F32(2) - F32(1)


def model_inputs_ref(pts, batch_idx, classes, scales, table, n_classes, lut, tlp=None, proj_size=2048):
    """pts float32 [M,8], batch_idx int32 [M], classes float32 [M], scales float32 [M,3]; table: model_of_class();
    lut {id: code}.  Returns {"models": {name: {...}} in upstream's order (a model without rows is absent),
    "abs_xyz" [N,3], "scales" [N,3], "index" [N]}."""
    cls = classes.astype(np.int64)
    assert np.array_equal(cls.astype(F32), classes) and cls.min(initial=0) >= 0 and cls.max(initial=0) < n_classes
    slot = np.asarray(table)[cls] if len(cls) else np.zeros(0, np.int8)
    models = {}
    for m, name in enumerate(MODELS):
        idx = slot == m
        if idx.sum() == 0:
            continue
        b = batch_idx[idx].copy()
        for i, bi in enumerate(np.unique(b)):      # "Make batch_idx contiguous and starts from 0"
            b[b == bi] = i
        p = pts[idx]
        c = classes[idx]
        onehots = np.zeros((len(c), n_classes), F32)
        onehots[np.arange(len(c)), c.astype(np.int64)] = 1
        zs = get_z(p[:, 4], lut)
        models[name] = {"index": np.nonzero(idx)[0].astype(np.int64), "pts": p, "abs_xyz": p[:, :3], "rel_xyz": p[:, 5:8],
                        "batch_idx": b.astype(np.int32), "classes": c, "scales": scales[idx], "onehots": onehots,
                        "proj_uv": projection_uv(p[:, :2], tlp, proj_size), "zs": zs,
                        "group": None if zs is None else groups_of(zs, len(c)),
                        "group_instances": None if zs is None else np.array(list(zs), np.int16),
                        "codes": None if zs is None else np.concatenate([v["z"] for v in zs.values()])}
    cat = lambda key, width: (np.concatenate([v[key] for v in models.values()]) if models  # noqa: E731
                              else np.zeros((0,) + width, F32))
    return {"models": models, "abs_xyz": cat("abs_xyz", (3,)), "scales": cat("scales", (3,)),
            "index": cat("index", ()).astype(np.int64)}


def gaussian_points_ref(xyz, scales, attrs):
    """get_gaussian_points on [N,3] arrays and the concatenated attribute dict -> [N,14]."""
    n = len(xyz)
    xyz = xyz + attrs["xyz"] if "xyz" in attrs else xyz
    scales = scales * attrs["scale"] if "scale" in attrs else scales
    opacity = attrs["opacity"] if "opacity" in attrs else np.ones((n, 1), F32)
    rot = np.concatenate([np.ones((n, 1), F32), np.zeros((n, 3), F32)], axis=1)
    return np.concatenate([xyz, opacity, scales, rot, attrs["rgb"]], axis=1).astype(F32)


# ---- the recorded reference (tests/golden/model_inputs.npz, written by tests/golden/make_model_inputs_golden.py) ----------
CLASS_IDS = {"GOOGLE_EARTH": {"BLDG_FACADE": 2, "BLDG_ROOF": 7}, "KITTI_360": {"BLDG_FACADE": 2, "BLDG_ROOF": 7, "CAR": 3}}
N_CLASSES = 8


def golden_cases(path):
    """{case: {key: array}} with the case prefix stripped."""
    cases = {}
    with np.load(path) as z:
        for key in z.files:
            case, rest = key.split("/", 1)
            cases.setdefault(case, {})[rest] = z[key]
    return cases


def golden_inputs(c):
    """A recorded case as model_inputs_ref's arguments (a dict of keyword arguments)."""
    present = [bool(v) for v in c["present"]]
    table = model_of_class(CLASS_IDS[str(c["dataset"])], N_CLASSES, *present)
    lut = {int(i): code for i, code in zip(c["lut_ids"], c["lut_codes"])}
    return dict(pts=c["pts"][0], batch_idx=c["batch_idx"][0, :, 0], classes=c["classes"][0, :, 0], scales=c["scales"][0],
                table=table, n_classes=N_CLASSES, lut=lut, tlp=c["tlp"] if c["tlp"].size else None,
                proj_size=int(c["proj_size"]))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
