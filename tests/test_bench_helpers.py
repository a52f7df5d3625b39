"""bench.py's pure helpers (no GPU): the `search_kernels` object SURVEY.md 8d asks for (search / feature / legal kernels as
microseconds per step and HBM GB/s), the counter summary behind it (tools/pmc_traffic.py), --dump-outputs and the legs --full
adds behind the timed steps."""
import csv
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_search_kernels_object_arithmetic():
    bench = _load("agz_bench", "bench.py")
    ms = {"k_pre": 40.0, "k_expand": 8.0, "k_scan": 1.0, "k_leaf_features": 4.0, "k_post": 4.0}      # summed over 100 steps
    d = {"evals": 819200, "steps": 100}
    pmc = {"k_pre": {"dispatches": 59, "FETCH_SIZE_bytes_per_dispatch": 20e6, "WRITE_SIZE_bytes_per_dispatch": 4e6},
           "k_leaf_features": {"dispatches": 59, "FETCH_SIZE_bytes_per_dispatch": 6e6, "WRITE_SIZE_bytes_per_dispatch": 84e6}}
    o = bench.search_kernels_object(ms, 100, d, games=1024, N=9, step_ms=46.0, pmc=pmc)
    assert o["steps_timed"] == 100 and o["leaves_per_step"] == 8192.0
    k = o["kernels"]
    assert abs(k["k_pre"]["us_per_step"] - 400.0) < 1e-9 and abs(k["k_pre"]["share_of_step"] - 0.4 / 46.0) < 1e-12
    assert abs(k["k_pre"]["pmc_gb_s"] - 24e6 / 400e-6 / 1e9) < 1e-9 and "algorithmic_gb_s" not in k["k_pre"]
    lf = k["k_leaf_features"]
    assert lf["algorithmic_bytes_per_step"] == 8192 * (8 * 81 + 128 * 81)           # features.jl:3-26: 8 boards in, [N*N][32] f32 out
    assert abs(lf["algorithmic_gb_s"] - lf["algorithmic_bytes_per_step"] / 40e-6 / 1e9) < 1e-6
    assert abs(lf["algorithmic_frac_of_hbm_peak"] - lf["algorithmic_gb_s"] / 8000.0) < 1e-12
    assert abs(o["us_per_step_total"] - 570.0) < 1e-9
    assert "pmc_gb_s" not in k["k_post"] and k["k_scan"]["algorithmic_bytes_per_step"] == 8192.0
    assert bench.search_kernels_object(ms, 0, d, 1024, 9, 46.0, None) is None


def test_counter_summary_lists_the_search_kernels(tmp_path):
    pt = _load("agz_pmc_traffic", os.path.join("tools", "pmc_traffic.py"))
    for counter, vals in (("FETCH_SIZE", {"agz::k_pre(agz::View)": [100.0, 300.0], "void agz::k_wino_gemm4<3, false, 64>(float const*)": [1000.0, 1000.0]}),
                          ("WRITE_SIZE", {"agz::k_pre(agz::View)": [10.0, 30.0], "void agz::k_wino_gemm4<3, false, 64>(float const*)": [500.0, 500.0]})):
        d = tmp_path / counter
        d.mkdir()
        with open(d / "x_counter_collection.csv", "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["Kernel_Name", "Counter_Name", "Counter_Value"])
            for k, vs in vals.items():
                for v in vs:
                    w.writerow([k, counter, v])
    s = pt.summarise(8192, 9, [str(tmp_path / "FETCH_SIZE"), str(tmp_path / "WRITE_SIZE")])
    assert s["tower_layer_dispatches"] == 2
    assert s["bytes_per_launch"] == 1024.0 * (2 * 1000.0 + 500.0)                    # FETCH doubled (16 B/lane streaming reads), KiB counters
    pre = s["search_kernels"]["k_pre"]
    assert pre["dispatches"] == 2 and pre["FETCH_SIZE_bytes_per_dispatch"] == 1024.0 * 200.0 and pre["WRITE_SIZE_bytes_per_dispatch"] == 1024.0 * 20.0


class _FakeEngine:
    """the slice of the Engine API bench.dump_outputs reads, with deterministic contents"""

    def __init__(self, games, N, nrec, moves):
        import types
        self.cfg, self.P, self.A = types.SimpleNamespace(games=games), N * N, N * N + 1
        self.nrec, self.moves = nrec, moves

    def debug_live_record(self, g):
        return (g * 5 + 3) % self.cfg.games + 100, 0          # (game id, moves so far): ids in another order than slots

    def tree_root(self, g):
        return 1000 + g

    def node_info(self, g, root):
        import types
        return types.SimpleNamespace(N=float(g), W=0.5 * g, Q=0.5)

    def node_floats(self, g, root, field):
        import numpy as np
        return np.arange(self.A, dtype=np.float32) * (field + 1) + g

    def node_board(self, g, root):
        import numpy as np
        return (np.arange(self.P) % 3 - 1).astype(np.int8)

    def stats(self):
        return {"steps": 7, "positions": 11, "evals": 13}

    def records(self):
        import numpy as np
        return [dict(game_id=k, num_moves=self.moves, result=1 - 2 * (k % 2), final_score=0.5 + k,
                     moves=np.arange(self.moves, dtype=np.int16), pis=np.full((self.moves, self.A), k, np.float32),
                     qs=np.full(self.moves, -k, np.float32)) for k in range(self.nrec)]


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path):
    import numpy as np
    bench = _load("agz_bench", "bench.py")
    eng = _FakeEngine(games=16, N=5, nrec=6, moves=10)
    shapes = bench.dump_outputs(eng, str(tmp_path / "all"))
    a = {p.stem: np.load(p) for p in (tmp_path / "all").iterdir()}
    assert set(a) == set(shapes) and all(list(a[k].shape) == shapes[k] for k in a)
    assert all(x.dtype in (np.float32, np.float64) and x.size > 0 for x in a.values())
    assert a["root_child_n"].shape == (16, 26) and (a["root_game_id"] == np.arange(16) + 100).all()
    # row k holds the game with the k-th smallest id: id 103 runs in slot 0, id 104 (row 4) in slot 13
    assert (a["root_prior"][3] == np.arange(26) * 3).all() and (a["root_nwq"][4] == [13, 6.5, 0.5]).all()
    assert (a["record_game_id"] == np.arange(6)).all() and a["record_pis"].shape == (60, 26)
    assert list(a["counters"]) == [13, 11, 7]                     # evals, positions, steps: keys in sorted order
    # no finished game yet (a short timed window): no record arrays at all, and no array is empty
    shapes = bench.dump_outputs(_FakeEngine(games=16, N=5, nrec=0, moves=10), str(tmp_path / "none"))
    assert not any(k.startswith("record_") for k in shapes) and all(np.prod(v) > 0 for v in shapes.values())
    assert sorted(p.stem for p in (tmp_path / "none").iterdir()) == sorted(shapes)
    # a budget too small for everything: a seeded sample, the same one every time, in slot / game-id order
    big = _FakeEngine(games=4096, N=9, nrec=200, moves=80)
    budget = 4 << 20
    for d in ("s1", "s2"):
        bench.dump_outputs(big, str(tmp_path / d), budget=budget)
    files = sorted((tmp_path / "s1").iterdir())
    assert sum(p.stat().st_size for p in files) <= budget
    for p in files:
        assert np.array_equal(np.load(p), np.load(tmp_path / "s2" / p.name))
    s = {p.stem: np.load(p) for p in files}
    assert 0 < len(s["root_game_id"]) < 4096 and (np.diff(s["root_game_id"]) > 0).all()
    assert 0 < len(s["record_game_id"]) < 200 and (np.diff(s["record_game_id"]) > 0).all()
    assert s["record_pis"].shape == (80 * len(s["record_game_id"]), 82)


def test_a_plain_run_adds_no_leg_and_full_adds_every_one_that_applies():
    bench = _load("agz_bench", "bench.py")
    parse = bench.arg_parser().parse_args
    every = {"live_traffic", "sustained", "alt_precision", "config_legs", "cpu_baseline"}
    assert bench.extra_legs(parse(["--steps", "20", "--warmup", "5"]), 1) == set()
    assert bench.extra_legs(parse(["--steps", "20", "--warmup", "5", "--no-cpu-baseline"]), 1) == set()
    assert bench.extra_legs(parse(["--full"]), 1) == every
    assert bench.extra_legs(parse(["--full", "--no-live-traffic", "--no-config-legs"]), 1) == every - {"live_traffic", "config_legs"}
    assert bench.extra_legs(parse(["--full", "--no-sustained", "--no-alt-precision", "--no-cpu-baseline"]), 1) == {"live_traffic", "config_legs"}
    # the live counter passes and the configs[3] / [4] legs belong to the headline workload, the f32s leg and the sustained
    # MFMA rates to exact-f32 runs; at N > 1 only the sustained rates remain
    assert bench.extra_legs(parse(["--full", "--board", "5", "--tower", "1"]), 1) == {"sustained", "alt_precision", "cpu_baseline"}
    assert bench.extra_legs(parse(["--full", "--stagger", "0"]), 1) == {"sustained", "alt_precision", "cpu_baseline"}
    assert bench.extra_legs(parse(["--full", "--precision", "f16"]), 1) == {"cpu_baseline"}
    assert bench.extra_legs(parse(["--full", "--gpus", "2"]), 2) == {"sustained"}
