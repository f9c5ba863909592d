#!/usr/bin/env python
"""Generates tests/golden/ffn_bits.json: the bits of the feed-forward operator (gcm_ffn_* and gcm_ffn_split_*, DESIGN.md
section 18) as the library built from one commit computes them, pinned for refactors of its kernels.  Per case the SHA-256
of the raw little-endian float32 bytes of y and of each of the seven gradients (null for a gradient that was not asked
for), and beside them the commit the library was built from and the hipcc and torch versions.  Hashes and settings only.

    python tests/golden/make_ffn_bits_golden.py <commit id of the sources the library was built from> [output path]

Needs a GPU and the built library.  It goes through gaussiancity_amd.ffn.layernorm_mlp_residual and tests/ffn_ref.py
(make_inputs, run) alone, so it runs unchanged on any commit that has the split entry points.  Run it again when the
arithmetic of the operator is changed on purpose or the toolchain moves; tests/test_ffn_bits_gpu.py imports the cases and
the hashing from here and compares.

Cases.  One-launch path: NARROW x NS, without a row scale and with scales(N).  Split path, split mode: NARROW + WIDE x NS,
the same two.  Split path, rows mode: per ROWS shape the smallest N the plan puts in rows mode (ffn.split_plan's limit
through ffn_split_plans.first_rows_mode_n), with scales(N).  Gradient subsets: both paths at SUBSET_SHAPE, SUBSET_N for
each of SUBSETS -- the two gating branches of the host's backward apart."""
import hashlib
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ffn_ref import EPS, LEAVES, TENSORS, make_inputs, run  # noqa: E402
from ffn_split_plans import first_rows_mode_n  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "ffn_bits.json")
NS = (1, 65, 257)
NARROW = ((4, 4), (32, 128), (48, 40), (128, 512))
WIDE = ((132, 528), (256, 1024), (512, 2048), (388, 200))
ROWS = ((32, 128), (132, 528), (256, 1024), (512, 2048))  # one per instantiation that rows mode reaches
SUBSET_SHAPE, SUBSET_N = (48, 40), 65
SUBSETS = (("x",), ("w2", "b2"))
SEED = 7000


def scales(N):
    """tests/test_ffn_split_gpu.py's row scale: dropped, kept and rescaled rows, the first three fixed."""
    s = torch.tensor([0.0, 1.0, 1.0 / 0.7])[torch.randint(0, 3, (N,), generator=torch.Generator().manual_seed(N))]
    s[0] = 0.0
    if N > 1:
        s[1] = 1.0 / 0.7
    if N > 2:
        s[2] = 1.0
    return s


def operator(split):
    def fn(t, s):
        from gaussiancity_amd.ffn import layernorm_mlp_residual
        return layernorm_mlp_residual(t["x"], t["ln_w"], t["ln_b"], EPS, t["w1"], t["b1"], t["w2"], t["b2"], s, split=split)
    return fn


def cases():
    """(label, split, N, C, Hd, scaled, need) in a fixed order; the label is the key in the file."""
    from gaussiancity_amd import ffn
    out = []
    for split, shapes in ((False, NARROW), (True, NARROW + WIDE)):
        for C, Hd in shapes:
            for N in NS:
                assert not split or ffn.split_plan(N, C, Hd)["mode"] == "split", (N, C, Hd)
                for scaled in (False, True):
                    out.append((split, N, C, Hd, scaled, LEAVES))
    for C, Hd in ROWS:
        N = first_rows_mode_n(Hd, ffn.split_plan(1, C, Hd)["limit"])
        assert ffn.split_plan(N, C, Hd)["mode"] == "rows" and ffn.split_plan(N - 1, C, Hd)["mode"] == "split", (N, C, Hd)
        out.append((True, N, C, Hd, True, LEAVES))
    for split in (False, True):
        for need in SUBSETS:
            out.append((split, SUBSET_N, *SUBSET_SHAPE, True, need))
    label = "%s C=%d Hd=%d N=%d %s need=%s"
    return [(label % ("split" if sp else "one-launch", C, Hd, N, "scaled" if sc else "plain", "+".join(need)), sp, N, C, Hd, sc, need)
            for sp, N, C, Hd, sc, need in out]


def digest(t):
    """SHA-256 of the tensor's float32 elements as little-endian bytes, row-major; None for no tensor."""
    if t is None:
        return None
    assert t.dtype == torch.float32
    return hashlib.sha256(t.contiguous().numpy().astype("<f4", copy=False).tobytes()).hexdigest()


def compute(dev, only=None):
    """{label: {tensor: digest}} for the cases whose label `only` accepts (all without it)."""
    got = {}
    for label, split, N, C, Hd, scaled, need in cases():
        if only is not None and not only(label):
            continue
        inp = make_inputs(N, C, Hd, SEED + N)
        res = run(operator(split), inp, dev, torch.float32, scales(N) if scaled else None, need=need)
        got[label] = {k: digest(res[k]) for k in TENSORS}
    return got


def hipcc_version():
    try:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the Makefile's default
        out = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout
        return next(line.strip() for line in out.splitlines() if "version" in line.lower())
    except (OSError, subprocess.CalledProcessError, StopIteration):
        return "unknown"


def main():
    if len(sys.argv) not in (2, 3):
        raise SystemExit("usage: make_ffn_bits_golden.py <commit id of the sources the library was built from> [output path]")
    if not torch.cuda.is_available():
        raise SystemExit("make_ffn_bits_golden needs a GPU")
    blob = {"commit": sys.argv[1], "hipcc": hipcc_version(), "torch": torch.__version__,
            "device": torch.cuda.get_device_name(0), "cases": compute(torch.device("cuda:0"))}
    out = sys.argv[2] if len(sys.argv) == 3 else PATH
    with open(out, "w") as f:
        json.dump(blob, f, indent=0, sort_keys=True)
        f.write("\n")
    print(out, os.path.getsize(out), "bytes,", len(blob["cases"]), "cases")


if __name__ == "__main__":
    main()
