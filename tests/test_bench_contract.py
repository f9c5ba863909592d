"""The bench line contract (driver + judge): checked on the committed lines under profiles/, which bench.py
produced on an MI355X, and on bench.py's argument surface (no GPU needed)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = {"metric": str, "value": (int, float), "unit": str, "n_gpus": int, "steps": int, "warmup": int,
            "ms_per_step": (int, float), "higher_is_better": bool, "scaling": str, "dtype": str, "data": str, "config": dict}


def _check(line, with_cpu=True):
    for k, t in REQUIRED.items():
        assert k in line and isinstance(line[k], t), k
    assert "vs_baseline" in line and line["vs_baseline"] is None          # BASELINE.md publishes no number
    assert "workload" in line["config"] and "model" not in line["config"]
    r = line["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    # "valu": the alpha-blend kernels are bound by VALU issue (VERDICT r01 item 4 asks for that roofline, with the
    # HBM accounting of SURVEY 8d beside it under "hbm")
    assert r["bound"] in ("hbm", "mfma", "valu") and r["unit"] in ("GB/s", "TFLOP/s", "G wave-instr/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    if r["bound"] == "valu":
        h = r["hbm"]
        assert h["unit"] == "GB/s" and abs(h["frac"] - h["achieved"] / h["peak"]) < 1e-3 and "traffic" in h
    if with_cpu:
        c = line["cpu_baseline"]
        for k in ("value", "unit", "cores", "kind", "sample"):
            assert k in c, k
        assert c["kind"] in ("reference", "port") and c["cores"] >= 1


def test_committed_bench_lines_follow_the_contract():
    for name, cpu in (("r01_bench_c3.json", True), ("r01_bench_visibility.json", True), ("r01_bench_grid_encoder.json", True),
                      ("r01_bench_c5.json", False), ("r02_bench_c3.json", True)):
        line = json.load(open(os.path.join(ROOT, "profiles", name)))
        _check(line, cpu)
    c3 = json.load(open(os.path.join(ROOT, "profiles", "r01_bench_c3.json")))
    assert c3["unit"] == "frames/s" and "5000000 Gaussians, 1920x1080" in c3["metric"] and c3["scaling"] == "weak"
    assert c3["cpu_baseline"]["gpu_image_bit_exact_vs_cpu"] is True
    assert json.load(open(os.path.join(ROOT, "profiles", "r01_bench_visibility.json")))["cpu_baseline"]["kind"] == "reference"
    r2 = json.load(open(os.path.join(ROOT, "profiles", "r02_bench_c3.json")))
    assert r2["cpu_baseline"]["gpu_image_bit_exact_vs_cpu"] is True and "C1" in r2["cpu_baseline"]
    sec = r2["secondary"]                     # C2 forward+backward: stats, per-stage bytes, K7 roofline, CPU baseline
    assert sec["unit"] == "ms/frame" and sec["roofline"]["kernel"] == "blend_bwd" and "frame_stats" in sec
    assert sec["cpu_baseline"]["gpu_image_bit_exact_vs_cpu"] is True
    assert sec["cpu_baseline"]["worst_gradient_error_over_max"] <= 1e-4


def test_bench_cli_surface():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--help"]).decode()
    for flag in ("--gpus", "--steps", "--warmup", "--config", "--path", "--train-step", "--full", "--dump-outputs"):
        assert flag in out


def test_dump_outputs_budget_and_sample(tmp_path):
    """--dump-outputs: float32 where exact (else float64), small arrays whole, 64 MB in all, the same sample every run."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    rng = np.random.default_rng(1)
    arrays = {"image": rng.random((3, 1080, 1920), dtype=np.float32), "radii": rng.integers(0, 99, 5_000_000, dtype=np.int32),
              "num_rendered": [123456789012], "big": rng.random(30_000_000, dtype=np.float32), "empty": np.zeros(0)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))}
    assert sorted(got) == ["big", "image", "num_rendered", "radii"]
    assert got["num_rendered"].dtype == np.float64 and got["num_rendered"][0] == 123456789012
    assert got["radii"].dtype == np.float32 and np.array_equal(got["radii"], arrays["radii"])
    assert got["image"].dtype == np.float32 and got["image"].size < arrays["image"].size
    assert np.isin(got["big"], arrays["big"]).all()
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET_BYTES
    for k, a in got.items():
        assert np.array_equal(a, np.load(str(tmp_path / "b" / (k + ".npy"))))


def test_round5_lines_and_the_static_scene_second_line():
    """The round's headline line is the stateless one; every line of the static scene's file says which of the two it is,
    and the pairs were taken on one box (same workload, the cached line faster, never the file the driver's command writes)."""
    def lines(name):
        return [json.loads(l) for l in open(os.path.join(ROOT, "profiles", name)) if l.startswith("{")]
    c3 = lines("r05_bench_c3.json")[-1]
    _check(c3, True)
    assert c3["config"]["cull"].startswith("stateless") and c3["cpu_baseline"]["gpu_image_bit_exact_vs_cpu"] is True
    assert c3["secondary"]["cpu_baseline"]["worst_gradient_error_over_max"] <= 1e-4
    both = lines("r05_bench_static_scene.jsonl")
    assert len(both) == 8
    for stateless, static in zip(both[0::2], both[1::2]):
        _check(stateless, False)
        _check(static, False)
        assert stateless["config"]["cull"].startswith("stateless") and static["config"]["cull"].startswith("STATIC SCENE")
        assert "second line" in static["config"]["cull"]
        assert stateless["config"]["workload"] == static["config"]["workload"] and stateless["metric"] == static["metric"]
        assert static["value"] > stateless["value"]
        assert static["stages_ms"]["preprocess"]["ms_single_stream"] < stateless["stages_ms"]["preprocess"]["ms_single_stream"]
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--help"]).decode()
    assert "--static-scene" in out and "--fast-exp" not in out
