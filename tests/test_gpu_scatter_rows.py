"""-m gpu: the tile-table rows laid out XCD class by XCD class (gcr_tt_row.h).  The count kernel and the scatter kernel
take their row from the same map; a map that is not a bijection of [0, NG) loses or duplicates a row of the table, and
with it instances.  The shapes here are the ones at which that shows: NG below 8, NG not a multiple of 8, and NG = 65
from G = 2 K1 blocks per group -- plus one frame that is band-sorted first.  None of it may change a bit: `ranges`, the
sorted lists, n_contrib, final_T and the image against the CPU oracle (whole forward state, test_gpu_parity's check)."""
import numpy as np
import pytest

import gpu_util as G
import scenes
from test_gpu_parity import _check_forward, _frame

pytestmark = pytest.mark.gpu


def _groups(P):
    """gcr_preprocess_grid + gcr_tile_table_groups (gcr_internal.h, gcr_binning.hip) for P below 512 * 512: K1 blocks of
    256 Gaussians, at most 128 groups of G consecutive blocks."""
    nblocks = (P + 255) // 256
    ng = min(128, nblocks)
    g = -(-nblocks // ng)
    return nblocks, g, -(-nblocks // g)


# P, blocks, G, NG, largest scale (the big frame's lists stay near the lazy sort's 1024 entries)
CASES = [(256, 1, 1, 1, 6.0), (1280, 5, 1, 5, 6.0), (2048, 8, 1, 8, 6.0), (3328, 13, 1, 13, 6.0), (33024, 129, 2, 65, 1.5)]


@pytest.mark.parametrize("P,nblocks,g,ng,smax", CASES, ids=["NG%d" % c[3] for c in CASES])
def test_every_row_of_the_table_is_counted_and_scattered_once(oracle_mod, cuda_device, P, nblocks, g, ng, smax):
    W, H = 160, 96  # 60 tiles
    assert _groups(P) == (nblocks, g, ng)
    rs = scenes.camera(W, H, pose_index=(40 + ng) % 24)._replace(sh_degree=1)
    sc = scenes.blob_scene(P, 40 + ng, 1, smax=smax)
    fr = _frame(oracle_mod, rs, sc)
    assert fr.R > 0 and (fr.ranges[:, 1] > fr.ranges[:, 0]).all()  # every tile has a segment to get wrong
    for train in (False, True):
        args, out = G.run_forward(rs, sc, cuda_device, for_backward=train)
        _check_forward(fr, G.decode(P, W, H, out), P, True)


def test_band_sorted_frame(oracle_mod, cuda_device):
    """The band sort renumbers the survivors before the table is counted: a workgroup's instances then fall into a few
    neighbouring tiles -- the rows are the same map.  (A band sort needs 256 tiles: 20 x 13 here.)"""
    from gaussiancity_amd import _native as N
    P, W, H = 33024, 320, 208
    assert _groups(P) == (129, 2, 65)
    rs = scenes.camera(W, H, pose_index=8)._replace(sh_degree=1)
    sc = scenes.blob_scene(P, 8, 1, smax=1.2)
    fr = _frame(oracle_mod, rs, sc)
    prev = N.set_option("band_sort_min", 0)  # every frame is band-sorted
    try:
        args, out = G.run_forward(rs, sc, cuda_device, for_backward=False)
    finally:
        N.set_option("band_sort_min", prev)
    L = N.get_layout(P, W, H, out[0])
    words = out[3][L.geom_num_rendered:L.geom_num_rendered + 128].cpu().numpy().view(np.uint64)
    assert words[9] != 0  # GCR_FRAME_BANDED: the table was counted over the band-sorted survivors
    _check_forward(fr, G.decode(P, W, H, out), P, True)
