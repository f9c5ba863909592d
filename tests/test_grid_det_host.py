"""Not gpu: the host side of the deterministic hash-grid table gradient (include/gce.h ABI v3) -- the workspace size
query, the argument checks of gce_backward_det (made before any HIP call), and which switch decides the path."""
import torch

from gaussiancity_amd import _native_e as E
from gaussiancity_amd import grid_encoder as GE

ROWS = 16 << 19  # GaussianCity's table: 16 levels x 2^19 rows


def test_workspace_size_query():
    lib = E.lib()
    q = lib.gce_backward_det_workspace_bytes
    n = 16 * 16384 * 32
    full = q(16384, 5, 16, ROWS)
    assert 16 * n <= full <= 18 * n  # two key and two id buffers, plus the histograms and the tile records
    sizes = [q(B, 5, 16, ROWS) for B in (1, 255, 256, 257, 4096, 16384)]
    assert sizes[0] > 0 and sizes == sorted(sizes)
    sizes = [q(3001, 3, L, 4096) for L in (1, 2, 5, 16, 32)]
    assert sizes[0] > 0 and sizes == sorted(sizes)
    assert q(8, 6, 2, 64) == 0 and b"D must be" in lib.gce_last_error()
    assert q(8, 3, 33, 64) == 0 and b"L must be" in lib.gce_last_error()
    assert q(1 << 22, 5, 16, ROWS) == 0 and b"2^31" in lib.gce_last_error()   # n = 2^31
    assert q((1 << 22) - 1, 5, 16, ROWS) > 0                                  # n just below
    assert q(8, 6, 2, 64) == 0 and lib.gce_last_error() != b""
    assert q(0, 5, 16, ROWS) == 0 and lib.gce_last_error() == b""             # valid and empty: no message


def _det(lib, dtype=E.DTYPE_F32, B=8, D=3, C=2, L=2, rows=64, ws=None, ws_bytes=0, ptr=None):
    return lib.gce_backward_det(dtype, ptr, ptr, ptr, ptr, rows, B, D, C, L, 1.0, 4, 0, None, None, 0, 0, ws, ws_bytes, None)


def test_backward_det_argument_checks_need_no_gpu():
    lib = E.lib()
    assert _det(lib) < 0 and b"workspace" in lib.gce_last_error()                     # NULL, 0 bytes
    need = lib.gce_backward_det_workspace_bytes(8, 3, 2, 64)
    buf = (torch.empty(need + 64, dtype=torch.uint8)).data_ptr()                       # host memory: never dereferenced
    assert _det(lib, ws=buf, ws_bytes=need - 1) == -1 and b"workspace" in lib.gce_last_error()
    assert _det(lib, ws=None, ws_bytes=need) == -1 and b"workspace" in lib.gce_last_error()
    assert _det(lib, dtype=7) == -3 and b"dtype" in lib.gce_last_error()              # GCE_ERR_UNSUPPORTED
    assert _det(lib, C=3) == -3 and b"C must be" in lib.gce_last_error()
    assert _det(lib, C=3, dtype=7) == -3 and b"C must be" in lib.gce_last_error()     # dims before dtype
    assert _det(lib, D=6) == -3 and b"D must be" in lib.gce_last_error()
    assert _det(lib, B=1 << 22, D=5, L=16) == -3 and b"2^31" in lib.gce_last_error()
    assert _det(lib, B=0) == 0                                                         # empty: nothing to do, no workspace
    assert _det(lib, B=0, dtype=7) == -3                                               # dtype before the empty case
    assert _det(lib, ws=buf, ws_bytes=need) == -1 and b"null tensor" in lib.gce_last_error()   # workspace before tensors


def test_deterministic_switch_precedence(monkeypatch):
    """explicit setting > GCE_DETERMINISTIC (read at import) > torch's deterministic-algorithms switch; default off."""
    before = torch.are_deterministic_algorithms_enabled()
    try:
        GE.set_deterministic(None)
        monkeypatch.setattr(GE, "_ENV_DETERMINISTIC", None)
        torch.use_deterministic_algorithms(False)
        assert GE.deterministic_enabled() is False
        torch.use_deterministic_algorithms(True)
        assert GE.deterministic_enabled() is True
        monkeypatch.setattr(GE, "_ENV_DETERMINISTIC", False)       # the environment overrides torch
        assert GE.deterministic_enabled() is False
        torch.use_deterministic_algorithms(False)
        monkeypatch.setattr(GE, "_ENV_DETERMINISTIC", True)
        assert GE.deterministic_enabled() is True
        GE.set_deterministic(False)                                 # the explicit setting overrides both
        assert GE.deterministic_enabled() is False
        monkeypatch.setattr(GE, "_ENV_DETERMINISTIC", False)
        GE.set_deterministic(True)
        assert GE.deterministic_enabled() is True
        GE.set_deterministic(None)
        assert GE.deterministic_enabled() is False
    finally:
        GE.set_deterministic(None)
        torch.use_deterministic_algorithms(before)


def test_set_deterministic_rejects_other_values_and_stats_have_both_counters():
    import pytest
    with pytest.raises(TypeError):
        GE.set_deterministic(1)
    assert GE.deterministic_enabled() in (False, True)
    GE.reset_stats()
    assert GE.stats() == {"atomic_backward_calls": 0, "deterministic_backward_calls": 0}
