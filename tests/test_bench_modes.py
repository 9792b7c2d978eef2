"""bench.py's two modes: a plain run prints the result line with the roofline read off the timed steps and nothing that
takes time of its own; --full adds the CPU baseline.  Small shapes, each run as a CHILD process."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--size", "128", "--batch", "2", "--steps", "2", "--warmup", "2"]


def run_bench(*extra):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["roofline"]["frac"] > 0 and out["roofline"]["avg_launch_ms"] > 0
    return out, r.stderr


def test_bench_help_lists_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-500:]
    assert "--full" in r.stdout and "--no-cpu-baseline" in r.stdout


@pytest.mark.gpu
def test_bench_plain_run_has_no_cpu_baseline():
    out, err = run_bench()
    assert "cpu_baseline" not in out
    assert "[cpu_baseline]" not in err


@pytest.mark.gpu
def test_bench_full_run_adds_cpu_baseline():
    out, _ = run_bench("--full")
    cb = out["cpu_baseline"]
    assert cb["value"] > 0 and cb["unit"] == "images/sec" and cb["kind"] == "port" and "@128x128" in cb["sample"]
    out, _ = run_bench("--full", "--no-cpu-baseline")
    assert "cpu_baseline" not in out
