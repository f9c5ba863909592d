"""A/B timing of the building generator's attribute head: the grouped kernels (gaussiancity_amd.attr_head) against a
torch-ops yardstick of upstream's per-instance loop, in one process, alternating.

  python tools/attr_head_bench.py [--reps 7] [--iters 5] [--out profiles/attr_head.jsonl]

The head is the building configuration's: in 124, 7 classes, hidden 512, z 256, no shared ModLinear (n_shared_layers
= 1), one `rgb` layer, fc_out_rgb.  Cases: N = 518 000 points under no_grad with 1, 16 and 256 instances, and N = 65 536
forward + backward (loss = out.sum()) with 1 and 16 instances; every point belongs to one instance, instances
interleaved at random.  The yardstick is written here against the method's behaviour (models/generator.py:382-430 and
ModLinear.forward): per instance a boolean-mask gather, alpha and beta by addmm, the modulated [1, 512, 512] weight,
baddbmm, the activation, fc_out, the transform and a boolean-mask scatter.  Both paths share the parameters; their
outputs (and, in the training cases, the gradient of the layer's weight) are compared before timing.  After a warm-up
of both: --reps rounds, in each one block of --iters yardstick calls and one block of --iters fused calls between
device events (the yardstick's host waits are inside its block: they are part of what it costs); the figure is the
median over the rounds of a block's time per call.  One JSON line per case and path.  Needs a GPU; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiancity_amd import attr_head  # noqa: E402

IN_DIM, CLASSES, HIDDEN, Z_DIM, FACTOR = 124, 7, 512, 256, 2.0
CASES = [("inference", 518000, 1), ("inference", 518000, 16), ("inference", 518000, 256),
         ("training", 65536, 1), ("training", 65536, 16)]


class ModLinear(torch.nn.Module):
    """Parameters under upstream's names; forward is ModLinear.forward with output_mode, mod_bias and no bias."""

    def __init__(self, in_features, out_features, style_features):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.randn(out_features, in_features) / in_features ** 0.5)
        self.bias, self.mod_bias, self.output_mode = None, True, True
        self.weight_alpha = torch.nn.Parameter(torch.randn(in_features, style_features) / style_features ** 0.5)
        self.bias_alpha = torch.nn.Parameter(torch.ones(in_features))
        self.weight_beta = torch.nn.Parameter(torch.randn(out_features, style_features) / style_features ** 0.5)
        self.bias_beta = torch.nn.Parameter(torch.zeros(out_features))

    def forward(self, x, z):
        z = z.reshape(z.shape[0], -1, z.shape[-1])
        alpha = torch.addmm(self.bias_alpha.unsqueeze(0), z.reshape(-1, z.shape[-1]), self.weight_alpha.t()).reshape(*z.shape[:-1], -1)
        beta = torch.addmm(self.bias_beta.unsqueeze(0), z.reshape(-1, z.shape[-1]), self.weight_beta.t()).reshape(*z.shape[:-1], -1)
        w = self.weight.unsqueeze(0) * alpha
        return torch.baddbmm(beta, x, w.transpose(1, 2))


class GaussianAttrMLP(torch.nn.Module):
    """The building head; forward is the yardstick: upstream's loop over the instances in torch ops."""

    def __init__(self):
        super().__init__()
        self.factors, self.n_layers, self.n_shared_layers = {"rgb": FACTOR}, {"rgb": 1}, 1
        self.act = torch.nn.LeakyReLU(negative_slope=0.2)
        self.fc_m_a, self.fc_1 = torch.nn.Linear(CLASSES, HIDDEN, bias=False), torch.nn.Linear(IN_DIM, HIDDEN)
        self.fc_2_rgb_0, self.fc_out_rgb = ModLinear(HIDDEN, HIDDEN, Z_DIM), torch.nn.Linear(HIDDEN, 3)

    def forward(self, pt_feat, onehots, zs):
        b, n, _ = pt_feat.size()
        f = self.act(self.fc_1(pt_feat) + self.fc_m_a(onehots))
        output = torch.zeros(b, n, 3, device=pt_feat.device)
        for v in zs.values():
            h = self.act(self.fc_2_rgb_0(f[v["idx"]].unsqueeze(0), v["z"]))
            output[v["idx"]] = (torch.sigmoid(self.fc_out_rgb(h)) - 0.5) * FACTOR
        return {"rgb": output}


def block_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attr_head.jsonl"))
    a = ap.parse_args()
    if a.reps < 5 or a.iters < 3:
        raise SystemExit("at least 5 blocks of 3 calls")
    if not torch.cuda.is_available():
        raise SystemExit("attr_head_bench needs a GPU")
    dev = torch.device("cuda:0")
    module = types.SimpleNamespace(GaussianAttrMLP=GaussianAttrMLP, ModLinear=ModLinear)
    yardstick = GaussianAttrMLP.forward
    attr_head.install(module)
    fused = GaussianAttrMLP.forward
    torch.manual_seed(2024)
    head = GaussianAttrMLP().to(dev)
    g = torch.Generator(device="cpu").manual_seed(2024)
    lines = []
    for mode, n, instances in CASES:
        feat = torch.randn(1, n, IN_DIM, generator=g).to(dev)
        onehots = torch.nn.functional.one_hot(torch.randint(0, CLASSES, (1, n), generator=g), CLASSES).float().to(dev)
        ids = torch.randint(0, instances, (1, n), generator=g).to(dev)
        zs = {i: {"z": torch.randn(1, Z_DIM, generator=g).to(dev), "idx": ids == i} for i in range(instances)}
        training = mode == "training"

        def call(method):
            if not training:
                with torch.no_grad():
                    return method(head, feat, onehots, zs)["rgb"]
            head.zero_grad(set_to_none=True)
            out = method(head, feat, onehots, zs)["rgb"]
            out.sum().backward()
            return out

        attr_head.reset_stats()
        got, want = call(fused).detach(), None
        grad = head.fc_2_rgb_0.weight.grad.clone() if training else None
        want = call(yardstick).detach()
        torch.cuda.synchronize()
        assert attr_head.stats()["fused_calls"] == 1, attr_head.stats()
        diff = float((got - want).abs().max())
        gdiff = float((grad - head.fc_2_rgb_0.weight.grad).abs().max() / head.fc_2_rgb_0.weight.grad.abs().max()) if training else 0.0
        if not (diff <= 1e-5 * FACTOR and gdiff <= 1e-4):
            raise SystemExit("the two paths disagree: output %g, weight gradient %g of its maximum" % (diff, gdiff))
        paths = {"yardstick": yardstick, "fused": fused}
        for method in paths.values():
            block_ms(lambda: call(method), a.iters)
        times = {p: [] for p in paths}
        for _ in range(a.reps):
            for p, method in paths.items():
                times[p].append(block_ms(lambda: call(method), a.iters))
        med = {p: statistics.median(t) for p, t in times.items()}
        flop = 2.0 * n * HIDDEN * HIDDEN * (3 if training else 1)   # the ModLinear layer's products alone
        for p in paths:
            rec = {"tool": "attr_head_bench", "mode": mode, "path": p, "device": torch.cuda.get_device_name(dev), "points": n,
                   "instances": instances, "in": IN_DIM, "hidden": HIDDEN, "z": Z_DIM, "reps": a.reps, "iters": a.iters,
                   "ms_per_call_median": round(med[p], 4), "ms_per_call_min": round(min(times[p]), 4),
                   "ms_per_call_max": round(max(times[p]), 4), "speedup_vs_yardstick": round(med["yardstick"] / med[p], 3),
                   "modlinear_layer_tflop": round(flop / 1e12, 4), "max_abs_diff_vs_yardstick": diff if p == "fused" else 0.0,
                   "weight_grad_diff_of_max": gdiff if p == "fused" else 0.0}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    attr_head.uninstall(module)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
