"""bench.py without --full does only what its headline figure needs: the line holds the contract keys and `config`, and
none of the records --full adds (profiled pass, contraction checks, other configurations, CPU baseline)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config"}


def test_plain_run_prints_the_headline_alone():
    n = 64
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--size", str(n)]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert set(line) == HEADLINE_KEYS
    assert line["metric"] == "pressure-Poisson V-cycles/sec" and line["unit"] == "V-cycles/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-9)
    assert line["config"]["cells"] == n ** 3
