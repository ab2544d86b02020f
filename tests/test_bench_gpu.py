"""bench.py's plain run (the headline figure only) on the GPU; the legs behind --full are not run."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_line_only(dev, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "2",
                        "--size", "128", "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"] == "detection train-step images/sec" and d["unit"] == "images/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 2
    assert d["value"] > 0 and d["ms_per_step"] > 0 and abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) < 0.01 * d["value"]
    for leg in ("fp32_exact", "reference_style_step", "config1_hip", "ddp", "crnn", "cpu_baseline"):
        assert leg not in d, leg
    assert "--full" in d["roofline"]["traffic_source"]  # (no live PMC passes)
    assert os.path.exists(tmp_path / "loss.npy") and os.path.exists(tmp_path / "state.out_conv.0.weight.npy")
