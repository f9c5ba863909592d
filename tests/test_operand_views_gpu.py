"""Every public operator, every tensor operand, every legal torch view of it: the bits of the dense, aligned twin, forward
and backward (tests/operand_views.py has the table and the assertions).  One test per registry entry; each runs the
entry's dense baseline once and then one view per run.  `-k gcm` (gca, gcs, gcv, gce) selects one library's entries.

Two documented exceptions are part of the table, not of this file: views an operator refuses by contract (asserted to
raise with the documented message), and the hash-grid table gradient, bit-reproducible only with set_deterministic,
which is how its entry runs.
"""
import pytest
import torch

import operand_views as OV

pytestmark = pytest.mark.gpu

_RAN = {}


def _run(op, dev):
    if op.id not in _RAN:
        _RAN[op.id] = None  # a sweep that raises stays recorded as not counted
        _RAN[op.id] = OV.sweep(op, dev)
    return _RAN[op.id]


@pytest.mark.parametrize("op", OV.REGISTRY, ids=["%s-%s" % (op.lib, op.id) for op in OV.REGISTRY])
def test_views_give_the_dense_twins_bits(cuda_device, op):
    ran = _run(op, cuda_device)
    assert ran == len(op.pairs()) and ran > 0, (op.id, ran, len(op.pairs()))
    torch.cuda.synchronize()


def test_sweep_ran_every_registered_view(cuda_device):
    """The count of (operator, operand, view) runs is the registry's: nothing is dropped at run time.  Entries that the
    selection left out so far run here."""
    counts = {}
    for op in OV.REGISTRY:
        try:
            counts[op.id] = _run(op, cuda_device)
        except AssertionError:
            counts[op.id] = None
    failed = [k for k, v in counts.items() if v is None]
    assert not failed, "these entries' sweeps fail (their own tests say why): %s" % ", ".join(failed)
    assert sum(counts.values()) == OV.registered_count() and len(counts) == len(OV.REGISTRY)
    print("operand views: %d operators, %d (operand, view) runs" % (len(counts), sum(counts.values())))
