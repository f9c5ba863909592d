"""A/B timing of the attribute head at inference: one launch per key (gaussiancity_amd.attr_chain) against the path that
runs without it, in one process, alternating.

  python tools/attr_chain_bench.py [--reps 7] [--iters 5] [--out profiles/attr_chain.jsonl]

Background head (zs None: in 128 and 192, 8 classes, hidden 512, one `rgb` Linear layer) at N = 518 000 and 16 384 points,
against the module's own torch ops, written here in upstream's order (models/generator.py:382-430: fc_1, fc_m_a, add,
LeakyReLU, clone, Linear, LeakyReLU, fc_out, the transform).  Building head (in 124, 7 classes, hidden 512, z 256, one
`rgb` ModLinear) at N = 518 000 with 1, 16 and 256 instances, against attr_head's layered path (torch fc_1 / fc_m_a / add /
activation, one modulated_linear launch, head_out): what runs with only attr_head installed.  Both paths share parameters
and inputs; their outputs are compared before timing.  After a warm-up of both: --reps rounds, in each one block of --iters
calls per path between device events; the figure is the median over the rounds of a block's time per call.  Bytes are
what each path's operators read and write by their shapes (every torch op reads its inputs and writes its output once;
weights once per call), not a counter.  One JSON line per case and path.  Needs a GPU; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

from attr_head_bench import ModLinear, block_ms  # noqa: E402
from gaussiancity_amd import attr_chain, attr_head  # noqa: E402

HIDDEN, Z_DIM, FACTOR = 512, 256, 2.0
# generator, in, classes, points, instances
CASES = [("background", 128, 8, 518000, 0), ("background", 192, 8, 518000, 0), ("background", 128, 8, 16384, 0),
         ("background", 192, 8, 16384, 0), ("building", 124, 7, 518000, 1), ("building", 124, 7, 518000, 16),
         ("building", 124, 7, 518000, 256)]


class GaussianAttrMLP(torch.nn.Module):
    """One `rgb` key; forward is the module's own method for zs None in torch ops (with codes the timed paths are attr_head's
    and attr_chain's, and this method is not reached)."""

    def __init__(self, in_dim, classes, codes):
        super().__init__()
        self.factors, self.n_layers, self.n_shared_layers = {"rgb": FACTOR}, {"rgb": 1}, 1
        self.act = torch.nn.LeakyReLU(negative_slope=0.2)
        self.fc_m_a, self.fc_1 = torch.nn.Linear(classes, HIDDEN, bias=False), torch.nn.Linear(in_dim, HIDDEN)
        self.fc_2_rgb_0 = ModLinear(HIDDEN, HIDDEN, Z_DIM) if codes else torch.nn.Linear(HIDDEN, HIDDEN)
        self.fc_out_rgb = torch.nn.Linear(HIDDEN, 3)

    def forward(self, pt_feat, onehots, zs):
        assert zs is None, "the bench's own method is the background head's"
        f = self.fc_1(pt_feat)
        f = f + self.fc_m_a(onehots)
        f = self.act(f)
        _f = f.clone()
        _f = self.act(self.fc_2_rgb_0(f))
        return {"rgb": (torch.sigmoid(self.fc_out_rgb(_f)) - 0.5) * FACTOR}


def bytes_moved(generator, n, i, k, instances):
    """{path: bytes} by the operators' shapes, float32."""
    nh, g = n * HIDDEN, max(instances, 1)
    weights = HIDDEN * (i + k + 1) + HIDDEN * HIDDEN + HIDDEN + 3 * HIDDEN + 3
    chain = n * (i + k) + n * 3 + weights
    first = (n * i + nh) + (n * k + nh) + 3 * nh + 2 * nh  # fc_1, fc_m_a, add, LeakyReLU
    if generator == "background":
        # clone, Linear, LeakyReLU, fc_out, then sigmoid, - 0.5, * factor on [N, 3]
        return {"torch": 4 * (first + 2 * nh + 2 * nh + 2 * nh + (nh + n * 3) + 6 * n * 3 + weights), "chain": 4 * chain}
    modulation = 2 * g * HIDDEN + n  # alpha and beta [G, H], the group vector
    layered = first + (nh + nh) + (nh + n * 3) + weights + modulation  # modulated_linear, head_out
    return {"layered": 4 * layered, "chain": 4 * (chain + modulation)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attr_chain.jsonl"))
    a = ap.parse_args()
    if a.reps < 5 or a.iters < 3:
        raise SystemExit("at least 5 blocks of 3 calls")
    if not torch.cuda.is_available():
        raise SystemExit("attr_chain_bench needs a GPU")
    dev = torch.device("cuda:0")
    module = types.SimpleNamespace(GaussianAttrMLP=GaussianAttrMLP, ModLinear=ModLinear)
    attr_head.install(module)
    before = GaussianAttrMLP.forward  # attr_head's: the layered path with codes, the module's own torch ops without
    attr_chain.install(module)
    chained = GaussianAttrMLP.forward
    g = torch.Generator(device="cpu").manual_seed(2026)
    lines = []
    for generator, in_dim, classes, n, instances in CASES:
        torch.manual_seed(2026)
        head = GaussianAttrMLP(in_dim, classes, instances > 0).to(dev)
        feat = torch.randn(1, n, in_dim, generator=g).to(dev)
        onehots = torch.nn.functional.one_hot(torch.randint(0, classes, (1, n), generator=g), classes).float().to(dev)
        zs = None
        if instances:
            ids = torch.randint(0, instances, (1, n), generator=g).to(dev)
            zs = {i: {"z": torch.randn(1, Z_DIM, generator=g).to(dev), "idx": ids == i} for i in range(instances)}
        other = "torch" if generator == "background" else "layered"
        paths = {other: before, "chain": chained}

        def call(method):
            with torch.no_grad():
                return method(head, feat, onehots, zs)["rgb"]

        attr_chain.reset_stats()
        attr_head.reset_stats()
        got, want = call(chained), call(before)
        torch.cuda.synchronize()
        assert attr_chain.stats() == {"chain_calls": 1, "passed_on_calls": 0}, attr_chain.stats()
        assert attr_head.stats() == ({"fused_calls": 1, "original_calls": 0} if instances else {"fused_calls": 0, "original_calls": 1})
        diff = float((got - want).abs().max())
        if not diff <= 1e-5 * FACTOR:
            raise SystemExit("the two paths disagree: output %g" % diff)
        del got, want
        for method in paths.values():
            block_ms(lambda: call(method), a.iters)
        times = {p: [] for p in paths}
        for _ in range(a.reps):
            for p, method in paths.items():
                times[p].append(block_ms(lambda: call(method), a.iters))
        med = {p: statistics.median(t) for p, t in times.items()}
        moved = bytes_moved(generator, n, in_dim, classes, instances)
        flop = 2.0 * n * ((in_dim + classes) * HIDDEN + HIDDEN * HIDDEN + 3 * HIDDEN)
        for p in paths:
            rec = {"tool": "attr_chain_bench", "generator": generator, "path": p, "device": torch.cuda.get_device_name(dev),
                   "points": n, "instances": instances, "in": in_dim, "classes": classes, "hidden": HIDDEN,
                   "z": Z_DIM if instances else None, "reps": a.reps, "iters": a.iters,
                   "ms_per_call_median": round(med[p], 4), "ms_per_call_min": round(min(times[p]), 4),
                   "ms_per_call_max": round(max(times[p]), 4), "speedup_vs_" + other: round(med[other] / med[p], 3),
                   "bytes_moved": moved[p], "head_tflop": round(flop / 1e12, 4),
                   "tflops_at_median": round(flop / 1e9 / med[p], 2), "max_abs_diff_vs_" + other: diff if p == "chain" else 0.0}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del head, feat, onehots, zs
        torch.cuda.empty_cache()
    attr_chain.uninstall(module)
    attr_head.uninstall(module)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
