"""Per-Gaussian gradient error against the state-consistent binary64 reference -- shared by the host tests
(test_grad_rows_host.py), the GPU tests (test_gpu_grad_rows.py) and tools/grad_rows.py.  No GPU in here.

The suite's usual gradient bar is one scalar per tensor, max|d| <= 1e-4 * max(1, max|ref|); the largest row of a tensor
is 10^3 .. 10^4 times the typical one, so that bar does not see most Gaussians ("Per-Gaussian gradient rows").  Here every
Gaussian is a row of its own:

    norm_i = max|ref_i|                       over the row of the tensor reshaped to [P, -1]
    floor  = 1e-3 * median(norm_i, norm_i > 0)
    e_i    = max|got_i - ref_i| / max(norm_i, floor)

and a tensor is summed up by the median, the 99th percentile and the maximum of e_i over the rows with norm_i > 0, plus
the number of rows whose reference is all zero and whose value is not (those must be exact zeros).

The reference is oracle.Frame64.from_frame(frame32).backward(): K7 and K8's statements in binary64 on the binary32
forward state, every discrete decision taken as binary32 takes it.  The forward state is pinned bit for bit on the GPU,
so what remains is what the backward itself answers for.  The bar of a GPU kernel is not a number chosen here: it is
M = 4 times what the binary32 ORACLE -- another binary32 evaluation of the same sums from the same state -- leaves
against that reference on the same scene and tensor, plus 1e-6 (`within`)."""
import functools

import numpy as np
import torch

import scenes

STATS = ("median", "p99", "max")
M = 4.0
ABS = 1e-6

# name -> (P, W, H, SH degree, seed, blob_scene keywords, isotropic, mode); images are no multiple of the 16-pixel tile.
# A anisotropic, B sparse SH3 isotropic, C dense isotropic, D overdraw (lists near 3 000, n_contrib above 1 000),
# E = A with precomputed colours (no dL_dsh), F = A with a precomputed covariance (no dL_dscale, no dL_drot).
SCENES = {
    "A": (2000, 125, 93, 1, 11, {}, False, "sh"),
    "B": (400, 125, 93, 3, 14, dict(smin=0.3, smax=8.0), True, "sh"),
    "C": (6000, 61, 67, 1, 19, dict(smin=0.3, smax=8.0), True, "sh"),
    "D": (6000, 61, 67, 3, 17, dict(smax=12.0), False, "sh"),
    "E": (2000, 125, 93, 1, 11, {}, False, "colour"),
    "F": (2000, 125, 93, 1, 11, {}, False, "cov3d"),
}
BG = (0.2, 0.45, 0.1)

# Kernel variants of the backward: name -> (per-call gcr_options, the forward's `for_backward` hint; None = its default).
# "wave_units": one wave per (work item, quadrant) instead of one workgroup per (tile, piece) item; "deterministic":
# per-Gaussian 64-bit fixed-point sums instead of float atomics (on the wave kernel); bwd_piece is clamped to 64..223,
# so "piece256" is one piece of 223 entries; "inference_hint": the forward was not told that a backward follows.
VARIANTS = {
    "default": ({}, None),
    "wave_units": (dict(bwd_wave_units=1), True),
    "deterministic": (dict(deterministic_backward=1), True),
    "piece64": (dict(bwd_piece=64), True),
    "piece256": (dict(bwd_piece=256), True),
    "inference_hint": ({}, False),
    "training_hint": ({}, True),
}
# Every scene under the default; every variant on A (ordinary lists) and D (lists near 3 000: a dozen pieces and more).
CASES = [(s, "default") for s in "ABCDEF"] + [(s, v) for s in "AD" for v in VARIANTS if v != "default"]
_NAMES = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot")


def row_stats(ref, got):
    """{"median", "p99", "max"} of e_i over the rows with a non-zero reference, "rows" (how many those are) and
    "spurious" (rows whose reference is all zero and whose value is not).  A NaN or Inf anywhere in `got` gives inf."""
    P = ref.shape[0]
    assert got.shape[0] == P and ref.size == got.size, (ref.shape, got.shape)
    r = np.asarray(ref, np.float64).reshape(P, -1)
    g = np.asarray(got, np.float64).reshape(P, -1)
    norm = np.abs(r).max(axis=1)
    nz = norm > 0
    if not nz.any():
        return dict(median=0.0, p99=0.0, max=0.0, rows=0, spurious=int((g != 0).any(axis=1).sum()))
    floor = 1e-3 * float(np.median(norm[nz]))
    with np.errstate(invalid="ignore"):
        e = (np.abs(g - r).max(axis=1) / np.maximum(norm, floor))[nz]
    if not np.isfinite(e).all():
        return dict(median=np.inf, p99=np.inf, max=np.inf, rows=int(nz.sum()), spurious=int((g[~nz] != 0).any(axis=1).sum()))
    return dict(median=float(np.median(e)), p99=float(np.percentile(e, 99)), max=float(e.max()), rows=int(nz.sum()),
                spurious=int((g[~nz] != 0).any(axis=1).sum()))


def limits(oracle_stats, m=M):
    """Item by item what a binary32 kernel may leave, from what the binary32 oracle leaves: m * statistic + 1e-6."""
    return {k: m * oracle_stats[k] + ABS for k in STATS}


def within(stats, oracle_stats, m=M):
    """The rule of the GPU tests: every statistic inside `limits`, and no value where the reference has an all-zero row."""
    lim = limits(oracle_stats, m)
    return stats["spurious"] == 0 and all(stats[k] <= lim[k] for k in STATS)


def report(tag, stats, oracle_stats, m=M):
    lim = limits(oracle_stats, m)
    return "%-24s " % tag + "  ".join("%s %.2e (oracle %.2e, limit %.2e)" % (k, stats[k], oracle_stats[k], lim[k])
                                      for k in STATS) + "  spurious %d" % stats["spurious"]


class Scene:
    """One scene of the table: inputs, the binary32 oracle's frame and gradients, the reference's gradients."""

    def __init__(self, O, name):
        P, W, H, deg, seed, kw, iso, mode = SCENES[name]
        self.name, self.P, self.W, self.H, self.mode = name, P, W, H, mode
        self.rs = scenes.camera(W, H, pose_index=seed % 24)._replace(sh_degree=deg, bg=torch.tensor(BG, dtype=torch.float32))
        sc = scenes.blob_scene(P, seed, deg, **kw)
        if iso:
            sc["scales"][:] = sc["scales"][:, :1]
        self.sc = sc
        self.use_sh = mode != "colour"
        inputs = dict(scenes.settings_kwargs(self.rs), means3D=sc["means3D"], opacities=sc["opacities"])
        inputs.update(dict(shs=sc["shs"]) if self.use_sh else dict(colors_precomp=sc["colors_precomp"]))
        geometry = dict(scales=sc["scales"], rotations=sc["rotations"])
        self.cov3D = None
        if mode == "cov3d":   # the covariance the oracle derives from scale and rotation, fed back precomputed
            self.cov3D = O.Frame(**inputs, **geometry).cov3D[:P].copy()
            geometry = dict(cov3D_precomp=self.cov3D)
        self.frame = O.Frame(**inputs, **geometry)
        self.dpix = np.random.default_rng(seed).normal(size=(3, H, W)).astype(np.float32)
        self.names = [n for n in _NAMES if not (n == "dL_dsh" and not self.use_sh)
                      and not (n in ("dL_dscale", "dL_drot") and mode == "cov3d")]
        self.g32 = self.frame.backward(self.dpix)
        self.ref = O.Frame64.from_frame(self.frame).backward(self.dpix)
        self.oracle_stats = {n: row_stats(self.ref[n], self.g32[n]) for n in self.names}
        for a in list(self.g32.values()) + list(self.ref.values()) + [self.dpix]:
            a.setflags(write=False)


def gpu_run(s, variant, device):
    """Forward and backward of scene `s` on the GPU under `variant`: (decoded forward state, the eight gradients)."""
    import gpu_util as G
    from gaussiancity_amd import ext
    opts, hint = VARIANTS[variant]
    with ext.options(**opts):
        args, out = G.run_forward(s.rs, s.sc, device, use_sh=s.use_sh, use_cov3d=s.cov3D is not None, cov3D=s.cov3D,
                                  for_backward=hint)
        state = G.decode(s.P, s.W, s.H, out)
        grads = G.run_backward(args, out, s.dpix.copy(), device)
    return state, grads


@functools.lru_cache(maxsize=None)
def _scene(O, name):
    return Scene(O, name)


def scene(O, name):
    """Built once per process and shared (read-only) by every test that asks for it."""
    return _scene(O, name)
