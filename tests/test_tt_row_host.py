"""gcr_tt_row (gaussiancity_amd/csrc/gcr_tt_row.h: the tile-table row of workgroup b of the tile-table kernels) on the
host -- gcc, the same header the device code includes: for every NG from 1 to 512 it is a permutation of [0, NG), and
the workgroups that share an L2 (equal b % 8) own consecutive rows.  A map that is not a bijection would make two
workgroups count into one row and leave another row unwritten: lost and duplicated instances."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XCDS = 8


def _rows():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "tt_row_check")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "gaussiancity_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tt_row_check.c"), "-o", exe])
    lines = subprocess.check_output([exe, "1", "512"]).decode().splitlines()
    assert len(lines) == 512
    return {ng: [int(v) for v in line.split()] for ng, line in zip(range(1, 513), lines)}


def test_rows_are_a_permutation_with_each_xcd_class_in_consecutive_rows():
    for ng, rows in _rows().items():
        assert len(rows) == ng and sorted(rows) == list(range(ng)), ng
        nxt = 0  # the classes follow each other in order, each one a run of consecutive rows in ascending b
        for c in range(min(XCDS, ng)):
            mine = [rows[b] for b in range(c, ng, XCDS)]
            assert mine == list(range(nxt, nxt + len(mine))), (ng, c)
            nxt += len(mine)
        assert nxt == ng
        # the closed form of the header's comment
        q, r = divmod(ng, XCDS)
        assert all(rows[b] == (b % XCDS) * q + min(b % XCDS, r) + b // XCDS for b in range(ng)), ng
