"""GPU: bench.py's own interface.  A plain run prints the headline line and nothing it does not need, `--steps` sets the timed
steps, `--dump-outputs DIR` writes what the last timed step computed (the same arrays from two runs with the same arguments), and
`--full` still adds the figures beyond the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernel_classes_ms_per_step", "fp32_exact", "c1", "c2", "c5", "cpu_baseline")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout                                    # ONE JSON line
    return json.loads(lines[0])


def test_plain_run_times_the_steps_asked_for_and_dumps_the_last_one(tmp_path):
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        out = _bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(d))
        assert all(k in out for k in HEADLINE) and out["higher_is_better"] is True and out["unit"] == "mel-frames/s"
        assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1 and out["value"] > 0
        assert abs(out["value"] - 8 * 1000 / (out["ms_per_step"] * 1e-3)) / out["value"] < 1e-3
        assert not [k for k in FULL_ONLY if k in out]
        assert sorted(os.listdir(d)) == ["mel.npy", "pcm.npy"]
        mel, pcm = np.load(d / "mel.npy"), np.load(d / "pcm.npy")
        assert mel.dtype == np.float32 and mel.shape == (8, 1000, 80) and np.isfinite(mel).all()
        assert pcm.dtype == np.float32 and pcm.shape == (8, 160 * 1000 + 32)
        assert np.array_equal(pcm, np.round(pcm)) and np.abs(pcm).max() <= 32768 and pcm.std() > 0     # int16 values, not silence
        dumps.append((mel, pcm))
    assert np.array_equal(dumps[0][0], dumps[1][0]) and np.array_equal(dumps[0][1], dumps[1][1])


def test_full_run_adds_the_figures_of_the_timed_region():
    out = _bench("--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-fp32-exact", "--no-c1", "--no-c2", "--no-c5")
    assert all(k in out for k in HEADLINE) and out["steps"] == 1
    rf = out["roofline"]
    assert rf["launches"] > 0 and rf["timed_launches"] > 0 and rf["achieved"] > 0 and "sclk_eff_mhz" in rf
    assert set(out["kernel_classes_ms_per_step"]) == {"attention", "adarmsnorm", "vocoder"}
    assert not [k for k in ("fp32_exact", "c1", "c2", "c5", "cpu_baseline") if k in out]
