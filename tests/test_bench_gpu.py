"""bench.py end to end on the GPU at a small size: a plain run carries the timed steps' figures alone, --full adds the legs
that take runs of their own (roofline profile, parity against the oracle; configs 2 / 3 and the CPU baseline are left out here
for time)."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "1", "--frames", "16"]
MOVED = ("roofline", "kernel_ms_per_step", "other_configs", "parity", "cpu_baseline", "gpu_over_cpu", "parity_ok")


def _bench(*args):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args], capture_output=True, text=True, timeout=600,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone():
    out = _bench()
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["unit"] == "clip-iters/s" and out["higher_is_better"] is True
    assert out["dtype"] == "bf16" and out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1
    assert not [k for k in MOVED if k in out]


def test_full_run_adds_roofline_and_parity():
    out = _bench("--full", "--no-other-configs", "--no-cpu-baseline")
    assert out["value"] > 0 and out["roofline"]["frac"] > 0 and out["roofline"]["launches_per_step"] > 0
    assert out["parity"]["ok"] and out["parity_ok"] is True
    assert "other_configs" not in out and "cpu_baseline" not in out
