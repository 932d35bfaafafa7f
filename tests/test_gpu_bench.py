"""bench.py with one GPU on a reduced HR size: a plain run carries the headline figure alone (plus what it derives from the
same timed steps); --full adds the blocks that take runs of their own.  The multi-rank forms are in test_gpu_sharded.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
def test_bench_plain_and_full(tmp_path, full):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--hr", "512",
           "--dump-outputs", str(tmp_path)]
    if full:
        cmd += ["--full", "--no-cpu-baseline"]  # the CPU baseline alone would take ~15 s
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["metric"] == "MAP gradient iterations/sec at fixed HR size" and out["unit"] == "MAP gradient iterations/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["value"] > 0 and abs(out["value"] * out["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert out["steps"] == 5 and out["warmup"] == 2 and out["config"]["timed_steps"] == 5
    assert out["full"] is full
    g = np.load(os.path.join(str(tmp_path), "grad.npy"))
    assert g.shape == (1, 512, 512) and g.dtype == np.float64 and np.isfinite(g).all()
    assert out["roofline"]["frac"] > 0 and out["cpu_baseline"] is None
    if full:
        assert out["roofline"]["hbm_fed"]["device_ms_per_step"] > 0
        assert out["f32"]["value"] > 0 and out["f32"]["dtype"] == "f32"
        assert out["cfg3"]["value"] > 0 and "configs[2]" in out["cfg3"]["workload"]
    else:
        assert out["roofline"]["hbm_fed"] is None
        assert "f32" not in out and "cfg3" not in out and "frames_variant" not in out
