"""-m gpu: bench.py's two shapes.  A plain run prints the headline line only; --full adds the per-stage times, the roofline and
the slot parity check against the CPU oracle, and leaves what the timed steps compute unchanged."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "3", "--warmup", "1", "--batch", "64", "--distinct", "8", "--preload", "5", "--settle", "5"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("stage_ms_per_batch", "roofline", "parity_checked_slots", "other_scenes", "host_fed", "cpu_baseline", "full_frontend",
             "per_frame_latency")


def _bench(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench(SMALL + ["--dump-outputs", str(tmp_path / "plain")])
    for k in HEADLINE:
        assert k in plain, k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 3 and plain["warmup"] == 1
    assert not [k for k in FULL_ONLY if k in plain]
    assert plain["dump_outputs"]["frames"] == 64

    full = _bench(SMALL + ["--full", "--no-extras", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    for k in HEADLINE:
        assert k in full, k
    assert full["roofline"]["kernel_ms"] > 0 and full["stage_ms_per_batch"]
    assert full["parity_checked_slots"] == 3 * 16          # 16 slots of each of the three contexts, all bit-exact
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) and len(names) == 6
    for n in names:
        assert np.array_equal(np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)), n
