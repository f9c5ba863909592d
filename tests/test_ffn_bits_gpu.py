"""-m gpu: a pin for refactors of the feed-forward operator (gcm_ffn_* and gcm_ffn_split_*).

tests/golden/ffn_bits.json holds, per case, the SHA-256 of the bytes of y and of the seven gradients as the library built
from the commit named in the file computed them.  The other tests compare the two paths with each other and with
float64, so a change that moves both paths together passes them; this one does not move.  Here the built library
recomputes every case of tests/golden/make_ffn_bits_golden.py (the cases and the hashing are imported from it) and every
hash must be equal: the one-launch path, the split path in split mode and in rows mode, and two gradient subsets on each
path.  No tolerance is involved.

The file is not a statement about the right value: when the operator's arithmetic is changed on purpose, or the toolchain
moves (the recorded hipcc and torch are printed on failure), regenerate it with the script and say so in the change."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_ffn_bits_golden", os.path.join(HERE, "golden", "make_ffn_bits_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_m
    _native_m.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(HERE, "golden", "ffn_bits.json")) as f:
        return json.load(f)


_ALL = "need=x+ln_w+ln_b+w1+b1+w2+b2"  # the end of a label whose case asks for all seven gradients
GROUPS = {"one-launch": lambda label: label.startswith("one-launch") and label.endswith(_ALL),
          "split": lambda label: label.startswith("split") and label.endswith(_ALL),   # split mode and rows mode
          "subsets": lambda label: not label.endswith(_ALL)}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_every_output_has_the_bits_the_pinned_commit_computed(dev, pinned, group):
    G = _generator()
    got = G.compute(dev, GROUPS[group])
    want = {k: v for k, v in pinned["cases"].items() if GROUPS[group](k)}
    assert got and set(got) == set(want), "the cases of the generator and of the file differ: %s" % sorted(set(got) ^ set(want))[:4]
    differing = [(label, k) for label in got for k in G.TENSORS if got[label][k] != want[label][k]]
    if differing:
        print("first differing case and tensor: %s, %s (%d of %d hashes differ)" % (*differing[0], len(differing), 8 * len(got)))
        print("pinned at commit %s with %s, torch %s on %s" % (pinned["commit"], pinned["hipcc"], pinned["torch"], pinned["device"]))
        print("here: torch %s, %s" % (torch.__version__, G.hipcc_version()))
    assert not differing, differing[0]
