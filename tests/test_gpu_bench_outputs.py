"""bench.py as the headline is measured: a plain `python bench.py --gpus 1 --steps K --warmup W` times exactly
K env.steps on the HIP library and runs nothing else, and `--dump-outputs DIR` writes what the last of them
returned — the same arrays from run to run, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("obs", "reward", "terminated", "truncated")


def _bench(out_dir, *args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--dump-outputs", str(out_dir), *args],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), {n: np.load(out_dir / f"{n}.npy") for n in NAMES}


@pytest.mark.gpu
def test_plain_bench_times_the_steps_and_dumps_the_same_outputs_twice(hip_lib, tmp_path):
    a = ("--steps", "5", "--warmup", "2", "--envs-per-gpu", "512", "--preheat", "30")
    line, out = _bench(tmp_path / "a", *a)
    again, out2 = _bench(tmp_path / "b", *a)
    assert line["data"] == "synthetic" and line["steps"] == 5 and line["windows"]["count"] == 1
    assert len(line["windows"]["kernel_ms_each"]) == 2 + 5 and line["ms_per_step"] > 0
    assert line["cpu_baseline"] is None and "secondary" not in line and "sustained" not in line
    assert out["obs"].shape == (512, 4) and out["obs"].dtype == np.float32 and np.isfinite(out["obs"]).all()
    assert out["reward"].shape == (512,) and out["reward"].dtype in (np.float32, np.float64)
    assert float(out["obs"].astype(np.float64).sum() + out["reward"].astype(np.float64).sum()) == pytest.approx(
        line["config"]["last_step_checksum"], rel=1e-12)
    for n in NAMES:
        np.testing.assert_array_equal(out2[n], out[n], err_msg=n)
    assert again["config"]["last_step_checksum"] == line["config"]["last_step_checksum"]
