"""bench.py's own surface: a plain run reports its timed steps and dumps what the last one returned; `--full` adds the
checks and per-kernel figures that take work of their own.  Tiny shapes: the workload itself is tests/test_model_gpu.py's."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
TINY = ["--slices", "4", "--size", "112", "--volumes", "2"]


def _bench(*args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MST_BENCH_SINGLE_DEVICE")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True, env=env, timeout=timeout)
    return r


@pytest.mark.parametrize("bad", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_an_empty_timing_window(bad):
    r = _bench(*bad, timeout=300)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr
    assert '"ms_per_step"' not in r.stdout


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_step(tmp_path):
    r = _bench("--steps", "3", "--warmup", "1", *TINY, "--dump-outputs", str(tmp_path / "out"))
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["metric"] == "volumes_per_sec_mst_dinov2_fwd" and line["unit"] == "volumes/s" and line["dtype"] == "bf16"
    assert abs(line["value"] - 2 / (line["ms_per_step"] * 1e-3)) < 0.01 * line["value"]
    assert line["parity_check"] is None and line["cpu_baseline"] is None and line["roofline"] is None and not line["kernels"]
    logits = np.load(tmp_path / "out" / "logits.npy")
    assert logits.dtype == np.float32 and logits.shape == (2, 2) and np.isfinite(logits).all()


@pytest.mark.gpu
def test_bench_full_run_keeps_its_extra_figures():
    r = _bench("--full", "--steps", "4", "--warmup", "1", *TINY)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 4 and line["ms_per_step"] > 0
    assert line["kernels"] and line["roofline"] and line["roofline"]["sampled_steps"] == 1
    assert line["cpu_baseline"]["value"] > 0
