"""bench.py end to end on a small workload (5x5, tower 1): a plain run prints the line read off its timed steps and nothing
that takes a run of its own; --full adds the f32s leg, the sustained MFMA rates and the CPU baseline (the live counter passes
and the configs[3] / [4] legs belong to the headline workload only: tests/test_bench_helpers.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--board", "5", "--tower", "1", "--readouts", "16", "--games", "16", "--steps", "5", "--warmup", "2", "--stagger", "0"]


def _line(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + SMALL + extra, capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_carries_only_what_its_timed_steps_measured():
    d = _line([])
    assert d["steps"] == 5 and d["warmup"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0 and d["dtype"] == "f32"
    assert d["roofline"]["launches_timed"] > 0 and "search_kernels" in d and "power" in d
    assert not {"cpu_baseline", "alt_precision", "config3", "config4", "generation"} & set(d)
    assert not {"sustained_mfma", "sustained_mfma_changing_operands"} & set(d["roofline"])


def test_full_run_adds_the_legs_that_take_runs_of_their_own():
    d = _line(["--full", "--cpu-baseline-seconds", "1"])
    assert d["steps"] == 5 and d["value"] > 0
    assert d["alt_precision"]["value"] > 0 and d["alt_precision"]["steps"] == 5
    assert d["roofline"]["sustained_mfma"]["value"] > 0 and d["roofline"]["sustained_mfma_changing_operands"]["value"] > 0
    assert d["cpu_baseline"]["value"] > 0
    assert "config3" not in d                     # (not the headline workload)
