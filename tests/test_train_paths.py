"""The GPU training tests (tests/test_gpu_train.py, tests/test_gpu_train_shapes.py) state which code path of
Trainer::step each of their batches takes.  train_paths (tests/train_twin.py) mirrors the host-side formulas that
choose it; this checks every statement against it, and that together the cases reach every path.  CPU only."""
from test_gpu_train import PATHS
from test_gpu_train_shapes import BATCH_CASE, DEAD_CASE
from train_twin import train_paths


def path(N, B):
    taps, wsplit, wchunk = train_paths(N, B)
    return ("taps" if taps else "direct"), wsplit, B * N * N - (wsplit - 1) * wchunk


def test_train_paths_mirrors_the_host_formulas():
    # conv3x3_direct_blocks = ceil(B N^2 / 128) * 2 workgroups; the tap split below 192 of them
    assert train_paths(9, 150)[0] and not train_paths(9, 151)[0]
    assert train_paths(19, 33)[0] and not train_paths(19, 34)[0]
    assert train_paths(9, 128) == (True, 4, 2592)                # 162 workgroups: NOT launch_conv3x3_direct
    assert train_paths(9, 170) == (False, 6, 2296)               # 13770 rows: the last split has 2290
    # the cap of 16 row splits starts at 39425 rows
    assert train_paths(5, 1576)[1] == 15 and train_paths(5, 1577)[1] == 16 and train_paths(9, 1000)[1] == 16
    for N in range(2, 20):
        for B in range(2, 700):
            taps, wsplit, wchunk = train_paths(N, B)
            M = B * N * N
            assert wchunk % 8 == 0 and 0 < M - (wsplit - 1) * wchunk <= wchunk    # every split has rows


def test_every_gpu_training_case_takes_the_path_it_claims():
    for (N, tower, B), claim in PATHS.items():
        assert path(N, B) == claim, ((N, tower, B), path(N, B), claim)
    assert path(DEAD_CASE[0], DEAD_CASE[2])[0] == "taps"
    N, _, batches = BATCH_CASE                         # and B = 170 is the direct branch at 9x9 with a ragged split
    assert [path(N, B) for B in batches] == [("taps", 1, 486), ("direct", 6, 2290), ("taps", 1, 648), ("taps", 2, 1616)]


def test_the_gpu_training_cases_reach_every_path():
    paths = {case: path(case[0], case[2]) for case in PATHS}
    wchunk = {case: train_paths(case[0], case[2])[2] for case in PATHS}

    def ragged(case):                                  # a last split shorter than wchunk and not a multiple of 8 rows
        branch, wsplit, last = paths[case]
        return wsplit > 1 and last < wchunk[case] and last % 8 != 0

    for branch in ("taps", "direct"):
        assert any(p[0] == branch and p[1] > 1 and ragged(c) for c, p in paths.items()), branch
        assert any(p[0] == branch for c, p in paths.items() if c[0] == 19), branch
    assert any(p[1] > 1 and p[2] == wchunk[c] for c, p in paths.items())          # full splits only
    assert any(p[1] == 16 and p[2] < wchunk[c] for c, p in paths.items())          # the cap, a short last split
    assert {c[0] for c in PATHS} >= {5, 7, 9, 13, 19}
    assert (19, 1, 2) in PATHS                                                    # the smallest batch, largest board
