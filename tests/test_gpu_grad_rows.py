"""-m gpu: every gradient tensor of the backward, Gaussian by Gaussian, against the state-consistent binary64 reference
(grad_rows.py; oracle.Frame64.from_frame).  The other GPU modules hold a tensor to 1e-4 * max|tensor|, which the largest
few rows decide; here the median, the 99th percentile and the maximum of the per-row relative error must each stay
within LIMIT times what the binary32 oracle itself leaves against the same reference on the same scene and tensor, plus
1e-6 -- and rows whose reference is all zero must be exact zeros.  No row is excluded.

The forward state is checked first (_check_forward: the oracle's bits), or the reference would not apply.

LIMIT is 4 for every (tensor, variant): GPU and oracle are two binary32 evaluations of the same sums from the same
state that differ in summation order (atomics, pieces, checkpoints instead of a division chain), in the moment form of
dL_dmean2D / dL_dconic and in the deterministic mode's fixed point, and a tail statistic over about 1 000 rows moves by
a small factor under reordering.  An entry of LIMITS above 4 is twice a measured ratio, never above 16, and names its
cause; tools/grad_rows.py writes the measured ratios to profiles/grad_rows.jsonl."""
import pytest

import grad_rows as GR
from test_gpu_parity import _check_forward

pytestmark = pytest.mark.gpu

# (tensor, variant) -> limit where rounding of the chosen summation form needs more than 4 (see the module docstring).
LIMITS = {
    # Measured 9.6 on the MAXIMUM of scene B (231 rows; median 0.8, p99 0.9: no term is dropped or mis-scaled), the same
    # in every run: one Gaussian.  dL_dscale is a linear function of that Gaussian's dL_dcov3D row, and on B the map
    # amplifies a row's relative error by up to 15 (3 at the median: cancellation between the covariance entries of a
    # small isotropic Gaussian under a non-unit quaternion); the GPU's dL_dcov3D of that scene is inside its own limit
    # (maximum 2.3 x the oracle's), and the oracle's own worst dL_dscale row of so few happens to be a mild one.  Twice the
    # measured ratio is 19.2; the limit stays at the cap.
    ("dL_dscale", "default"): 16.0,
    # Measured 5.85 on the MAXIMUM of scene D (1 138 rows; median 0.84, p99 0.96: no term is dropped or mis-scaled), one
    # Gaussian, the same bits in every run.  The deterministic mode is the wave kernel with a fixed-point flush, and the
    # wave kernel with float atomics is at 1.5 on the same scene and tensor: the rest is the quantum of the second
    # moments of a Gaussian whose tile rectangle is most of the image (gcr_det_frac_bits sizes that class for
    # pixels x d^2 x 64), amplified by the 1 / det^2 of K8's dL_dcov3D.  Twice the measured ratio.
    ("dL_dcov3D", "deterministic"): 11.7,
}


@pytest.mark.parametrize("name,variant", GR.CASES, ids=["%s-%s" % c for c in GR.CASES])
def test_every_gaussians_gradient_against_the_state_consistent_reference(oracle_mod, cuda_device, name, variant):
    """Measured on an MI355X (worst GPU : oracle ratio per case over the eight tensors, median / p99 / max; all of it in
    profiles/grad_rows.jsonl and DESIGN.md section 3):

    * every scene under the default kernel, and wave_units, piece64, piece256 and both hints on A and D: at most
      0.9 / 1.3 / 3.7 (the maximum: dL_dmean3D of A and F, one Gaussian, 2.7 to 3.7 over thirty runs of the workgroup kernel
      and 1.3 to 1.7 on the wave kernel; the next largest is 2.8), bar the dL_dscale entry of LIMITS;
    * with the checkpoints the forward left before this module existed (prefix colours; accum_rec of a piece as the
      difference C_final - C_prefix) the same cases stood at 10 / 190 / 500 on A and 33 / 410 / 1 100 on D
      (profiles/grad_rows_prefix_checkpoints.jsonl) -- the defect this module found;
    * the deterministic mode, with the binary points it had before this module (two classes, at most 32 fractional
      bits, a stale factor 8 max(W, H) in both bounds), stood at 0.7 / 17 / 12 (dL_dcolor, A), 1.1 / 57 / 27
      (dL_dcolor, D) and 18 to 19 on the maximum of dL_dmean2D / dL_dmean3D: beyond 16, a defect, fixed with three
      classes and up to 44 bits (gcr_internal.h).  Now at most 0.9 / 2.8 / 2.1 on A and D, bar its entry of LIMITS."""
    s = GR.scene(oracle_mod, name)
    state, got = GR.gpu_run(s, variant, cuda_device)
    _check_forward(s.frame, state, s.P, s.use_sh, has_cov3d_state=s.cov3D is None)
    failed = []
    for n in s.names:
        assert got[n].shape == s.g32[n].shape, n
        st, m = GR.row_stats(s.ref[n], got[n]), LIMITS.get((n, variant), GR.M)
        print(GR.report("%s %s %s" % (name, variant, n), st, s.oracle_stats[n], m))
        if not GR.within(st, s.oracle_stats[n], m):
            failed.append(n)
    assert not failed, failed
