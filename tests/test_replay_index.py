"""The replay arena's host-side game index (alphago.jl_amd/csrc/agz_replay_index.h) on the CPU:
tests/hostsim/replay_index_check.cpp drives it and a naive model -- a list of games, everything recomputed from scratch
-- with a few thousand seeded random operations and compares the five vectors, the counts, the window, the drop
decisions and the upload slices after each.  The program counts that the index was non-empty after at least half of the
operations and that the half-the-bytes rule dropped games at least 20 times, and fails otherwise.  Built plain and under
-fsanitize=address,undefined (a program of its own with both runtimes linked into it), and both are run."""
import os
import subprocess

import pytest

import hs
from test_explore import _static_sanitizer_runtimes


def _build_and_run(tmp_path, sanitize):
    exe = str(tmp_path / ("replay_index_check_san" if sanitize else "replay_index_check"))
    cmd = ["make", "-s", "-C", os.path.join(hs.HERE, "hostsim"), "replay_index_check", "REPLAY_INDEX_OUT=" + exe]
    r = subprocess.run(cmd + (["REPLAY_INDEX_SAN=1"] if sanitize else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "replay index check passed" in r.stdout and "FAILED" not in r.stdout and "ERROR" not in r.stderr


def test_index_equals_the_naive_model_plain(tmp_path):
    _build_and_run(tmp_path, sanitize=False)


def test_index_equals_the_naive_model_under_the_sanitizers(tmp_path):
    if not _static_sanitizer_runtimes():
        pytest.skip("no g++ with static libasan / libubsan")
    _build_and_run(tmp_path, sanitize=True)
