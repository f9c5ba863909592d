"""Not gpu: the state-consistent binary64 reference (oracle.Frame64.from_frame) and the per-Gaussian statistic of
grad_rows.py, before any kernel is held to them.

1. The reference is the same FUNCTION as the suite's independent formulation: on the scenes of test_oracle.py it equals
   dense_f64's autograd gradients to that module's 2e-4 * max.
2. The binary32 oracle stays close to it on scenes A..F of grad_rows.SCENES: per tensor, maximum 1e-3, 99th percentile
   2e-4 and median 5e-6 of the per-row relative error, all-zero rows exact.  These are not tolerances on code under test:
   the GPU's bar is four times the oracle's own statistic (test_gpu_grad_rows.py), and these conditions keep that bar
   from going loose.  A scene that misses them gets another seed (B did: seed 13 left one dL_dopacity row at 1.4e-3;
   seed 14 is the next), never another condition.  Measured here: worst maximum 7.1e-4 (dL_dcov3D, scene D), worst
   99th percentile 1.1e-4 (same), worst median 2.1e-6 (same).
3. Mutation sensitivity -- the gap this closes.  Three wrong gradients that today's per-tensor bar (_check_grads of
   test_gpu_parity.py) lets through and the per-row rule does not: a uniform relative bias of 1e-5, one lower-quartile
   Gaussian's covariance gradients zeroed, two similar Gaussians' dL_dmean3D exchanged."""
import numpy as np
import pytest
import torch

import grad_rows as GR
import scenes
import test_oracle as TO
from test_gpu_parity import _check_grads


# ---------------------------------------------------------------- 1. the same function as dense_f64
@pytest.mark.parametrize("name,deg,mode,bg,seed", TO.CASES, ids=[c[0] for c in TO.CASES])
def test_reference_equals_the_autograd_formulation(oracle_mod, name, deg, mode, bg, seed):
    W, H, P = 44, 36, 120
    rs = scenes.camera(W, H, pose_index=seed)._replace(sh_degree=deg, bg=torch.tensor(bg))
    sc = scenes.blob_scene(P, seed, deg)
    fr = TO._frame(oracle_mod, rs, sc, mode)
    dpix = np.random.default_rng(seed).normal(size=(3, H, W)).astype(np.float32)
    g = oracle_mod.Frame64.from_frame(fr).backward(dpix)
    assert all(v.dtype == np.float64 for v in g.values())
    _, _, gd = TO._dense(rs, sc, mode, dpix)
    pairs = [("means3D", "dL_dmean3D"), ("means2D", "dL_dmean2D"), ("opacities", "dL_dopacity"),
             ("scales", "dL_dscale"), ("rotations", "dL_drot")]
    pairs.append(("shs", "dL_dsh") if mode == "sh" else ("colors_precomp", "dL_dcolor"))
    for kd, ko in pairs:
        ref, got = gd[kd], g[ko].reshape(gd[kd].shape)
        assert np.abs(ref - got).max() <= 2e-4 * max(1.0, np.abs(ref).max()), kd


def test_reference_with_precomputed_cov3d_equals_the_autograd_formulation(oracle_mod):
    W, H, P = 40, 40, 90
    rs = scenes.camera(W, H)._replace(sh_degree=1)
    sc = scenes.blob_scene(P, 3, 1)
    cov = TO._frame(oracle_mod, rs, sc).cov3D[:P].copy()
    fr = TO._frame(oracle_mod, rs, sc, cov3D=cov)
    dpix = np.random.default_rng(0).normal(size=(3, H, W)).astype(np.float32)
    g = oracle_mod.Frame64.from_frame(fr).backward(dpix)
    _, _, gd = TO._dense(rs, sc, "sh", dpix, cov3D=cov)
    ref = gd["cov3D_precomp"]
    assert np.abs(ref - g["dL_dcov3D"]).max() <= 2e-4 * max(1.0, np.abs(ref).max())


def test_reference_takes_its_state_and_decisions_from_the_binary32_frame(oracle_mod):
    """The reference runs no forward: it carries the binary32 frame's state, and the frame is left as it was.  A
    binary64 frame of its own re-decides alpha < 1/255 and power > 0; on scene D that moves some rows by far more than
    rounding, which is what the state-consistent reference exists to avoid -- here it only has to differ from it."""
    s = GR.scene(oracle_mod, "D")
    fr = s.frame
    before = {k: getattr(fr, k).copy() for k in ("means2D", "conic_opacity", "final_T", "n_contrib", "point_list")}
    f64 = oracle_mod.Frame64.from_frame(fr)
    assert f64.state32 and not fr.state32 and f64.R == fr.R and f64.final_T.dtype == np.float64
    for k in ("means2D", "conic_opacity", "final_T", "n_contrib", "point_list", "ranges", "radii", "clamped", "rgb", "cov3D"):
        np.testing.assert_array_equal(getattr(f64, k), getattr(fr, k))
    g = f64.backward(s.dpix)
    for k in s.names:
        np.testing.assert_array_equal(g[k], s.ref[k])      # deterministic, and the switch does not leak between calls
    for k, v in before.items():
        np.testing.assert_array_equal(getattr(fr, k), v)
    g32 = fr.backward(s.dpix)
    for k in s.names:
        assert np.array_equal(g32[k].view(np.uint32), s.g32[k].view(np.uint32)), k


# ---------------------------------------------------------------- 2. the binary32 oracle against the reference
def test_row_statistic_on_a_hand_made_tensor():
    ref = np.array([[1.0, -2.0], [0.0, 0.0], [1e-6, 0.0], [4.0, 0.0], [0.0, 0.0]])
    got = np.array([[1.0, -2.2], [0.0, 0.0], [2e-6, 0.0], [4.0, 0.0], [0.0, 1e-30]])
    st = GR.row_stats(ref, got)
    # norms 2, 1e-6, 4 -> median 2 -> floor 2e-3: the tiny row is measured against the floor, not against itself
    assert st["rows"] == 3 and st["spurious"] == 1
    assert st["max"] == pytest.approx(0.1) and st["median"] == pytest.approx(1e-6 / 2e-3)
    assert GR.row_stats(ref, ref) == dict(median=0.0, p99=0.0, max=0.0, rows=3, spurious=0)
    bad = got.copy()
    bad[3, 1] = np.nan
    assert GR.row_stats(ref, bad)["max"] == np.inf
    assert GR.row_stats(np.zeros((3, 2)), np.zeros((3, 2)))["rows"] == 0
    assert GR.within(dict(median=4e-6, p99=1e-5, max=1e-4, spurious=0), dict(median=1e-6, p99=1e-5, max=1e-4))
    assert not GR.within(dict(median=6e-6, p99=1e-5, max=1e-4, spurious=0), dict(median=1e-6, p99=1e-5, max=1e-4))
    assert not GR.within(dict(median=0.0, p99=0.0, max=0.0, spurious=1), dict(median=1e-6, p99=1e-5, max=1e-4))


@pytest.mark.parametrize("name", sorted(GR.SCENES))
def test_binary32_oracle_stays_close_to_the_reference(oracle_mod, name):
    s = GR.scene(oracle_mod, name)
    fr = s.frame
    assert (fr.n_contrib > 0).mean() > 0.5, "the scene must cover the image"
    if name == "D":
        assert (fr.ranges[:, 1] - fr.ranges[:, 0]).max() > 2900 and fr.n_contrib.max() > 1000
    assert ("dL_dsh" in s.names) == (name != "E") and ("dL_dscale" in s.names) == ("dL_drot" in s.names) == (name != "F")
    for n in s.names:
        st = s.oracle_stats[n]
        print("%s %-12s median %.2e  p99 %.2e  max %.2e  rows %d" % (name, n, st["median"], st["p99"], st["max"], st["rows"]))
    for n in s.names:
        st = s.oracle_stats[n]
        assert st["rows"] > 200, n
        assert st["spurious"] == 0, n
        assert st["max"] <= 1e-3 and st["p99"] <= 2e-4 and st["median"] <= 5e-6, (n, st)


# ---------------------------------------------------------------- 3. what the per-tensor bar does not see
def _nonzero_rows_by_norm(a):
    norm = np.abs(a.reshape(a.shape[0], -1)).max(axis=1)
    idx = np.flatnonzero(norm > 0)
    return idx[np.argsort(norm[idx], kind="stable")]


def _mutants(s):
    g = {n: s.g32[n].copy() for n in s.names}
    yield "bias_1e-5", {n: (v * np.float32(1 + 1e-5)).astype(np.float32) for n, v in g.items()}
    by_norm = _nonzero_rows_by_norm(g["dL_dcov3D"])
    i = by_norm[len(by_norm) // 4]
    m = {n: v.copy() for n, v in g.items()}
    for n in ("dL_dcov3D", "dL_dscale", "dL_drot"):
        m[n][i] = 0
    yield "lower_quartile_row_zeroed", m
    by_norm = _nonzero_rows_by_norm(g["dL_dmean3D"])
    i, j = by_norm[len(by_norm) // 4], by_norm[len(by_norm) // 4 + 1]
    m = {n: v.copy() for n, v in g.items()}
    m["dL_dmean3D"][[i, j]] = m["dL_dmean3D"][[j, i]]
    yield "two_similar_rows_exchanged", m


@pytest.mark.parametrize("name", ["C", "D"])
def test_mutants_pass_the_per_tensor_bar_and_fail_the_per_row_rule(oracle_mod, name):
    s = GR.scene(oracle_mod, name)
    assert all(GR.within(s.oracle_stats[n], s.oracle_stats[n]) for n in s.names)   # the unmutated oracle passes its own rule
    seen = []
    for tag, m in _mutants(s):
        _check_grads(s.g32, m, s.names)                                  # today's bar: passes
        failing = [n for n in s.names if not GR.within(GR.row_stats(s.ref[n], m[n]), s.oracle_stats[n])]
        print(name, tag, "fails the per-row rule in", failing)
        assert failing, tag
        seen.append(tag)
    assert len(seen) == 3
